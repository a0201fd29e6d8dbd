"""CPU: the float64 restatement of the segmentation loss's mask term (tests/_seg_loss_util.py) against the REAL reference
(tests/golden/seg_loss.npz, tools/make_seg_loss_golden.py), the crop arithmetic of csrc/seg_loss.hip restated in fp32 against the reference's
stored crop masks, the mutants, the ``synthetic-seg`` generator and the refusals of ``YOLO(<-seg>).train`` before any device use."""
import numpy as np
import pytest
import torch

from tests import _loss_util as LU
from tests import _seg_loss_util as U


def _ref_grads(g, n_levels):
    return [torch.from_numpy(g[f"gc{i}"]).double() for i in range(n_levels)], torch.from_numpy(g["gp"]).double()


@pytest.mark.parametrize("cid", U.CASE_IDS)
def test_restatement_reproduces_the_reference(cid):
    """seg and its contribution to the total, and the gradients w.r.t. coefficient maps and prototypes, under the reference's own owner map:
    within the case's bars (16 x the fp32 reference's own error against its float64 run)."""
    case, owner, (seg, contrib, gc, gp) = U.case_reference(cid)
    g = U.golden(cid)
    assert np.array_equal(g["fg"], g["tscore"] > 0) and np.array_equal(g["fg"], g["owner"] >= 0)  # the foreground condition of every reference case
    det_total = float(g["items"][[0, 2, 3]].sum()) * case["gt"].shape[0]
    got = torch.tensor([float(g["items"][1]), float(g["total"]) - det_total], dtype=torch.float64)
    bi, bg = U.bars(cid)
    e_seg = LU.item_err(got[:1], seg.view(1))
    # the reference's total carries the other three items: the contribution is compared at the total's own magnitude
    e_tot = abs(float(g["total"]) - (det_total + float(contrib))) / max(abs(float(g["total"])), LU.ITEM_FLOOR)
    print(cid, "seg", float(seg), "reference", float(g["items"][1]), "err", e_seg, e_tot, "bar", bi)
    assert e_seg <= bi and e_tot <= max(bi, 4 * LU.F32_EPS)
    if cid in U.VARIANT_IDS:
        return
    rc, rp = _ref_grads(g, len(case["coefs"]))
    e_grad = LU.grad_err([*rc, rp], [*gc, gp])
    print(cid, "gradients err", e_grad, "bar", bg)
    assert e_grad <= bg
    if int((owner >= 0).sum()) == 0:
        assert float(seg) == 0 and all(not bool(t.any()) for t in (*gc, gp))


@pytest.mark.parametrize("cid", U.CASE_IDS)
def test_kernel_crop_arithmetic_equals_the_reference_crop_masks(cid):
    """ceil / clamp on the fp32 grid box (what the kernel computes) == crop_mask's comparisons, pixel for pixel, for every positive."""
    case, owner, _ = U.case_reference(cid)
    g = U.golden(cid)
    ref = np.unpackbits(g["crop"])[: int(np.prod(g["crop_shape"]))].reshape(g["crop_shape"]).astype(bool)
    pos = U.positives(owner)
    assert ref.shape[0] == len(pos)
    if not pos:
        return
    box = torch.stack([case["gt"][b, gi, 1:5] for b, _, gi in pos])
    mhw = tuple(case["proto"].shape[2:])
    assert np.array_equal(U.kernel_crop32(box, case["hw"], mhw).numpy(), ref)
    assert np.array_equal(U.reference_crop32(box, case["hw"], mhw).numpy(), ref)


def test_edge_cases_sit_on_the_comparisons():
    """edge0: the pixel at x1m is in, the pixel at x2m is out; one ulp inward drops column x1m, one ulp outward adds column x2m."""
    box = torch.tensor([[8.0, 12.0, 40.0, 36.0]])
    m0 = U.kernel_crop32(box, (64, 64), (16, 16))[0]
    assert m0[3:9, 2:10].all() and int(m0.sum()) == 6 * 8
    inward = torch.tensor([[LU._ulp(8.0, 1), LU._ulp(12.0, 1), LU._ulp(40.0, -1), LU._ulp(36.0, -1)]])
    outward = torch.tensor([[LU._ulp(8.0, -1), LU._ulp(12.0, -1), LU._ulp(40.0, 1), LU._ulp(36.0, 1)]])
    assert int(U.kernel_crop32(inward, (64, 64), (16, 16)).sum()) == 5 * 7 and int(U.kernel_crop32(outward, (64, 64), (16, 16)).sum()) == 7 * 9
    case = U.build_case("thin")
    assert int(U.kernel_crop32(case["gt"][0, :1, 1:5], case["hw"], (32, 32)).sum()) == 0  # no whole column inside


@pytest.mark.parametrize("mut", U.MUTANTS)
def test_every_mutant_is_caught(mut):
    caught = []
    for cid in U.ALL_IDS:
        case, owner, ref = U.case_reference(cid)
        seg, contrib, gc, gp = U.seg_from_owner64(case, owner, mut=(mut,))
        if not U.check_result(cid, torch.stack((seg, contrib)), gc, gp)["ok"]:
            caught.append(cid)
    print(mut, "caught by", caught)
    assert caught, f"no case tells a kernel with defect {mut!r} from a correct one"


def test_overlap_hidden_label_costs_loss_and_thin_counts_in_nfg():
    case, owner, (seg, _, gc, _) = U.case_reference("overlap")
    assert not bool((case["masks"][0] == 3).any()) and bool((owner[0] == 2).any())  # row 2 is nowhere in the map and owns anchors
    drop = owner.clone()
    drop[0][owner[0] == 2] = -1
    assert float(U.seg_from_owner64(case, drop)[0]) != float(seg)
    case, owner, (seg, _, gc, _) = U.case_reference("thin")
    thin_rows = [(b, a) for b, a, g in U.positives(owner) if (b, g) in ((0, 0), (1, 0))]
    pm = torch.cat([c.reshape(2, U.NM, -1) for c in gc], 2)
    assert len(thin_rows) == 3 and all(not bool(pm[b, :, a].any()) for b, a in thin_rows)  # empty crops: no gradient ...
    fewer = owner.clone()
    for b, a in thin_rows:
        fewer[b, a] = -1
    assert abs(float(U.seg_from_owner64(case, fewer)[0]) * 2 - float(seg) * 5) < 1e-12  # ... but they count in n_fg (5 against 2)


def test_synthetic_seg_generator():
    from drone_yolo_amd.engine.trainer import load_dataset, synthetic_overlap_masks

    d = load_dataset("synthetic-seg:6", 64, 10, 0)
    plain = load_dataset("synthetic:6", 64, 10, 0)
    assert d["masks"].shape == (6, 16, 16) and d["masks"].dtype == torch.uint8 and torch.equal(d["img"], plain["img"])
    assert d["bboxes"].shape == plain["bboxes"].shape and torch.equal(d["batch_idx"].sort().values, plain["batch_idx"].sort().values)
    for i in range(6):
        sel = d["batch_idx"] == i
        area = (d["bboxes"][sel][:, 2] * d["bboxes"][sel][:, 3])
        assert bool((area[:-1] >= area[1:]).all())  # labels stored largest first: value k + 1 is the image's k-th label
        assert int(d["masks"][i].max()) <= int(sel.sum())
    # the smaller label wins where two overlap, whatever order the labels came in
    img = torch.zeros(1, 3, 64, 64, dtype=torch.uint8)
    pair = dict(img=img, batch_idx=torch.zeros(2), cls=torch.tensor([[3.0], [7.0]]), bboxes=torch.tensor([[0.5, 0.5, 0.25, 0.25], [0.5, 0.5, 0.75, 0.75]]))
    out = synthetic_overlap_masks(pair, 16, 16)
    assert out["cls"].flatten().tolist() == [7.0, 3.0] and out["bboxes"][0, 2] == 0.75  # the larger one is label 0 now
    m = out["masks"][0]
    assert int(m[8, 8]) == 2 and int(m[8, 3]) == 1 and int(m[0, 0]) == 0 and int((m == 2).sum()) == 12 and int((m == 1).sum()) > 60


def test_train_refusals_leave_the_model_on_the_cpu(tmp_path):
    import drone_yolo_amd as D

    y = D.YOLO("yolov8n-seg.yaml")
    from drone_yolo_amd.engine.trainer import load_dataset

    good = load_dataset("synthetic-seg:4", 64, 10, 0)
    no_masks = {k: v for k, v in good.items() if k != "masks"}
    floats = dict(good, masks=torch.zeros(int(good["bboxes"].shape[0]), 16, 16))
    ratio3 = dict(good, masks=torch.zeros(4, 5, 5, dtype=torch.uint8))
    yaml_path = tmp_path / "set.yaml"
    yaml_path.write_text("path: .\ntrain: images\nval: images\nnames: [a]\n")
    for kw, word in ((dict(data="synthetic:4"), "masks"), (dict(data=no_masks), "masks"), (dict(data=floats), "overlap_mask"), (dict(data=ratio3), "prototype grid"),
                     (dict(data=good, device_augment=True), "device_augment"), (dict(data=str(yaml_path)), "YAML")):
        with pytest.raises(NotImplementedError, match="train") as e:
            y.train(epochs=1, imgsz=64, **kw)
        assert word in str(e.value), (word, str(e.value))
        assert y.trainer is None
    assert next(y.model.parameters()).device.type == "cpu"
    with pytest.raises(NotImplementedError, match="train"):
        y.model.init_criterion()
    # the P2 model's prototype grid is twice the quarter-size map: accepted by the same check
    from drone_yolo_amd.engine.trainer import check_seg_train_data

    check_seg_train_data(good, {}, 4.0)
    check_seg_train_data(good, {}, 8.0)
    check_seg_train_data("synthetic-seg:4", {}, 8.0)
    for m, where in ((y.model.model[-1], "forward_train"), (y.model.model[-1].proto, "proto_train")):
        m.train()
        with pytest.raises(NotImplementedError, match=where):
            m(torch.zeros(1, 3, 8, 8))
    y.model.eval()
