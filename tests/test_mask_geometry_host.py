"""CPU: the geometry sweep's cases (tests/_mask_util.py::PM_CASES, run on the device by tests/test_mask_geometry_gpu.py) are sound before any
GPU run, and the bar ``wrong == 0`` would catch the faults ``dy_process_mask`` could plausibly have.

Conditions per case (conditions, not measurements: a seed that fails one is replaced by the next, the condition is never loosened):
a correct fp32 implementation (``fp32_masks``: the reference's chain of torch ops on the CPU) differs from the float64 reference on no pixel
outside the unsure set; the unsure share is at most 1e-3 of the in-box pixels (the cap of tests/golden/seg.npz's fixtures); a case with
fewer than 1000 in-box pixels has no unsure pixel at all; the reference has set pixels, so a kernel that returns zeros cannot pass.
"""
import numpy as np
import pytest

from tests._mask_util import PM_TAGS, _args, case_reference, check_masks, degenerate_boxes, edges_clear, fp32_masks, make_boxes, pm_case, reference_masks


@pytest.mark.parametrize("tag", PM_TAGS)
def test_case_conditions(tag):
    inp, (ref, unsure, inbox) = case_reference(tag)
    T, (oh, ow) = sum(inp["counts"]), inp["out_hw"]
    assert ref.shape == unsure.shape == inbox.shape == (T, oh, ow) and ref.dtype == unsure.dtype == inbox.dtype == np.bool_
    res = check_masks(fp32_masks(*_args(inp)), ref, unsure, inbox)
    print(tag, res, "in-box", int(inbox.sum()))
    assert res["wrong"] == 0, f"{tag}: the fp32 chain differs from float64 on {res['wrong']} pixels outside the unsure set"
    assert res["unsure_share"] <= 1e-3
    if inbox.sum() < 1000:
        assert not unsure.any()
    assert res["set"] > 0


def test_case_table_is_the_stated_geometry():
    """What each case is there to hit, restated from its numbers."""
    P = {t: pm_case(t)["out_hw"][0] * pm_case(t)["out_hw"][1] for t in PM_TAGS}
    T = {t: sum(pm_case(t)["counts"]) for t in PM_TAGS}
    assert P["R1"] == 6 and P["R2"] == 15 and T["R2"] == 9  # no aligned group; 9 masks of 15 bytes start at every residue mod 8
    assert sorted({(t * 15) % 8 for t in range(9)}) == list(range(8))
    assert pm_case("R3")["out_hw"][1] < 8 and pm_case("R4")["out_hw"][1] == 9 and P["R4"] % 2 == 1
    for t in ("R5", "R5d", "R6", "D4"):  # downscaling on both axes
        c = pm_case(t)
        sh, sw = (c["window"] or (0, 0, *c["grid"]))[2:]
        assert sh > c["out_hw"][0] and sw > c["out_hw"][1]
    assert pm_case("R5")["window"][0] > 0 and pm_case("R5")["window"][1] > 0 and pm_case("R5")["counts"][1] == 0
    assert pm_case("R7a")["window"][2:] == (1, 1) and pm_case("R7b")["window"][2] == 1
    assert -(-P["R8"] // 8192) == 5 and P["R8"] % 8 != 0 and -(-P["R9"] // 8192) == 48  # runs of kPixPerBlock = 8192 pixels per mask
    assert pm_case("D1")["out_hw"][1] % 8 == 4 and (pm_case("D1")["out_hw"][0] * pm_case("D1")["out_hw"][1]) % 8 == 0
    c = pm_case("D2")
    assert c["out_hw"][1] / c["grid"][1] != c["out_hw"][0] / c["grid"][0] and (c["out_hw"][1] / c["grid"][1]) % 1
    # the degenerate boxes: D1's full image holds all seven, R5d's first image the first six
    for t, k in (("D1", 7), ("R5d", 6)):
        inp, (ref, _, _) = case_reference(t)
        b, d = pm_case(t)["degenerate"]
        assert d == k and inp["counts"][b] == pm_case(t)["max_det"]
        bx = inp["boxes"][b, inp["counts"][b] - d : inp["counts"][b]]
        assert bx[0, 2] < bx[0, 0] and bx[1, 2] < 0 and bx[3, 0] == bx[3, 2] and np.isnan(bx[5, 0]) and abs(bx[4]).min() == np.float32(1e30)
        m = ref[sum(inp["counts"][:b]) + inp["counts"][b] - d :][:d]
        assert m[4].any() and not m[[0, 1, 2, 3, 5]].any()  # the whole-image box has a mask, the others are empty
        if k == 7:
            assert not m[6].any()  # narrower than a proto pixel, between two integer columns


def test_make_boxes_keeps_the_edges_clear():
    rng = np.random.default_rng(5)
    for ratio, (w, h) in (((0.25, 0.25), (52, 40)), ((1.0, 1.0), (3, 2)), ((0.25, 0.25), (208, 160))):
        b = make_boxes(rng, 64, w, h, ratio)
        assert b.dtype == np.float32 and b.shape == (64, 4) and edges_clear(b, ratio)
        side = np.stack([(b[:, 2] - b[:, 0]) / w, (b[:, 3] - b[:, 1]) / h])
        ctr = np.stack([(b[:, 2] + b[:, 0]) / (2 * w), (b[:, 3] + b[:, 1]) / (2 * h)])
        assert side.min() >= 0.3 - 1e-5 and side.max() <= 0.9 + 1e-5 and ctr.min() >= 0.1 - 1e-5 and ctr.max() <= 0.9 + 1e-5
    assert not edges_clear(np.array([[4.0, 1.3, 9.3, 7.3]]), (0.25, 0.25))


def test_checker_counts():
    ref = np.zeros((2, 3, 4), bool)
    ref[0, 1, 1:3] = True
    unsure = np.zeros_like(ref)
    unsure[0, 1, 1] = True
    inbox = np.zeros_like(ref)
    inbox[0, 1] = True
    got = ref.copy()
    got[0, 1, 1] = False  # differs inside the unsure set
    got[1, 2, 3] = True  # differs outside it, and outside every box
    assert check_masks(got.astype(np.uint8), ref, unsure, inbox) == {"wrong": 1, "differ_in_unsure": 1, "unsure_share": 0.25, "set": 2}


# ---- the bar catches the faults the kernel could plausibly have --------------------------------------------------------------------
def _mutants(tag):
    """name -> the float64 reference with one fault built in."""
    inp, (ref, _, _) = case_reference(tag)
    T, (oh, ow) = ref.shape[0], inp["out_hw"]
    out = {}
    # the crop's left edge one pixel further right (a proto pixel in the default form, an output pixel otherwise)
    moved = inp["boxes"].copy()
    moved[..., 0] += 1.0 / (inp["ratio"][0] if inp["ratio"] else 1.0)
    out["crop edge moved by one pixel"] = reference_masks(*_args({**inp, "boxes": moved}))[0]
    out["half-pixel offset left out"] = reference_masks(*_args(inp), half_pixel=False)[0]
    out["x1 not clamped at sw - 1"] = reference_masks(*_args(inp), clamp_x1=False)[0]
    m = ref.copy().reshape(T, -1)
    m[1, :7] = False
    out["first 7 bytes of the second mask cleared"] = m.reshape(ref.shape)
    m = ref.copy()
    for t in range(T):  # a bounding region one row too tight at the lower edge: the mask's last row is stored as zeros
        rows = np.flatnonzero(m[t].any(1))
        if len(rows):
            m[t, rows[-1]] = False
    out["last row of the bounding region cleared"] = m
    return out


def _x1_can_pass_the_window(tag):
    """Whether any output column's right corner i0 + 1 lies beyond sw - 1 before the clamp (only when the x axis is not shrunk by 2x or more)."""
    c = pm_case(tag)
    sw, ow = (c["window"] or (0, 0, *c["grid"]))[3], c["out_hw"][1]
    src = np.maximum((np.arange(ow) + 0.5) * (np.float32(sw) / np.float32(ow)).astype(np.float64) - 0.5, 0.0)
    return bool((np.minimum(np.floor(src), sw - 1) + 1 > sw - 1).any())


@pytest.mark.parametrize("tag", ["R3", "R6", "D1"])
def test_checker_flags_mutations(tag):
    _, (ref, unsure, inbox) = case_reference(tag)
    assert check_masks(ref, ref, unsure, inbox)["wrong"] == 0
    for name, mutant in _mutants(tag).items():
        wrong = check_masks(mutant, ref, unsure, inbox)["wrong"]
        print(tag, name, wrong)
        if name.startswith("x1 not clamped") and not _x1_can_pass_the_window(tag):
            # R3 (8 -> 5 columns) and R6 (158 -> 41) shrink the x axis: the last source column is below sw - 1 and the clamp never acts,
            # so this mutation IS the reference there; D1 (13 -> 52) is the case that has to flag it
            assert tag in ("R3", "R6") and np.array_equal(mutant, ref)
            continue
        assert wrong > 0, f"{tag}: '{name}' passes the bar"


def test_degenerate_boxes_need_no_edge_clearance():
    """Their masks are the same for every rounding of their edges: moving every finite edge by +-0.25 pixel changes no reference pixel."""
    for tag in ("D1", "R5d"):
        inp, (ref, _, _) = case_reference(tag)
        b, d = pm_case(tag)["degenerate"]
        k = inp["counts"][b]
        assert np.array_equal(inp["boxes"][b, k - d : k], degenerate_boxes(*((pm_case(tag)["in_hw"] or inp["out_hw"])[::-1]), inp["ratio"] or (1.0, 1.0))[:d], equal_nan=True)
        t0 = sum(inp["counts"][:b]) + k - d
        for shift in (-0.25, 0.25):
            moved = inp["boxes"].copy()
            moved[b, k - d : k] += shift  # x and y edges alike: the masks are empty or whole whatever they are
            got = reference_masks(*_args({**inp, "boxes": moved}))[0]
            assert np.array_equal(got[t0 : t0 + d], ref[t0 : t0 + d])
