"""CPU: the Detect decode sweep's cases (tests/_detect_util.py, run on the device by tests/test_detect_geometry_gpu.py) are sound
before any GPU run.  Conditions, not measurements: the float64 restatement agrees with the oracle; every storage value survives
SiLU in both 16-bit types, so conv3x3_hhead's logits are exact; every logit is one exact fp32 number; the cases hold the peaks, the
halves, the flat rows and the exact ties they are named for; and at both confidence thresholds every image of every case has
anchors that pass, anchors that fail and (nc > 1) anchors that only the class mask removes, with at most 1 % of the anchors
inside the band conf (1 +- m) that the device comparison leaves out.
"""
import numpy as np
import pytest
import torch

from oracle import drone_yolo_oracle as O
from tests import _detect_util as U

ALL = {c.name: c for c in U.decode_cases() + U.head_cases() + U.hhead_cases()}
SWEEPS = {"decode": U.decode_cases, "head": U.head_cases, "hhead": U.hhead_cases}


def test_restatement_agrees_with_the_oracle_on_gaussian_logits():
    g = torch.Generator().manual_seed(5)
    for nc in (1, 10, 80):
        feats = [torch.randn(U.BATCH, 64 + nc, h, w, generator=g, dtype=torch.float64) * 2.5 for h, w in U.LEVELS]
        y64, y32 = U.ref_decode(feats, U.STRIDES, nc), O.detect_decode([f.float() for f in feats], U.STRIDES, nc)
        assert y64.shape == y32.shape == (U.BATCH, 4 + nc, sum(h * w for h, w in U.LEVELS))
        e = U.errors(y32, y64)
        print(nc, e)
        # fp32 against float64: a few ulps of the largest coordinate (25 cells x stride 4 and its like: 2^-17), of a probability
        assert e["xy"] <= 1e-4 and e["wh"] <= 1e-4 and e["sc"] <= 1e-6
        # and the restatement run in fp32 is the oracle's arithmetic up to the order of its sums
        e = U.errors(U.ref_decode(feats, U.STRIDES, nc, torch.float32), y64)
        assert e["xy"] <= 1e-4 and e["wh"] <= 1e-4 and e["sc"] <= 1e-6


def test_silu_rounds_back_to_every_storage_value():
    used = np.unique(np.concatenate([x.numpy().ravel() for c in ALL.values() if c.x is not None for x in c.x]))
    assert used[0] == 0.0 and used[1] >= 20.0 and used[-1] <= 60.0 and len(used) > 100
    for dt in (torch.bfloat16, torch.float16):
        assert np.array_equal(torch.from_numpy(used).to(dt).double().numpy(), used), f"{dt}: a storage value is off the grid"
        assert np.array_equal(U.silu_round_trip(used, dt), used), f"{dt}: SiLU moves a storage value"
    # the whole bfloat16 grid of [20, 60], not only the values drawn
    grid = torch.arange(20.0, 60.0 + 1e-9, 0.125, dtype=torch.float64).to(torch.bfloat16).double().unique().numpy()
    for dt in (torch.bfloat16, torch.float16):
        assert np.array_equal(U.silu_round_trip(grid, dt), grid)


@pytest.mark.parametrize("name", sorted(ALL))
def test_logits_are_exact_fp32_numbers_and_one_product_plus_bias(name):
    c = ALL[name]
    src, bias = U.class_affine(c.nc)
    for i, f in enumerate(c.feats):
        assert torch.equal(f.float().double(), f)
        if c.x is None:
            assert float(f[:, :64].max()) == 60.0 and float(f[:, :64].min()) <= -60.0  # the spread that underflows exp2
            continue
        x = c.x[i]
        assert torch.equal(U.S * x[:, :64] + U.B0, f[:, :64])
        assert torch.equal(U.S * x[:, 64:][:, src] + torch.from_numpy(bias).view(1, -1, 1, 1), f[:, 64:])
        near = f[:, : 64 + min(c.nc, 80)]
        assert bool(((near == -20.0) | ((near >= -10.0) & (near <= 10.0))).all())  # {-20} U [-10, 10]; classes 80.. sit FAR below


@pytest.mark.parametrize("family", U.FAMILIES)
def test_families_hold_what_they_are_named_for(family):
    c = U.make_case(family, 10)
    d = torch.cat([(U.reference(c)[:, :4, a0 : a0 + h * w] / s) for (h, w), s, a0 in zip(c.shapes, c.strides, np.cumsum([0] + [h * w for h, w in c.shapes]))], 2)
    wh = d[:, 2:4]  # left + right, top + bottom, in cells
    box = torch.cat([f[:, :64].reshape(U.BATCH, 4, 16, -1) for f in c.feats], 3)
    e = torch.softmax(box, 2)
    dist = (e * torch.arange(16.0, dtype=torch.float64).view(1, 1, 16, 1)).sum(2)
    if family == "peak":
        # the 15 other bins weigh exp(-30) each: 120 exp(-30) = 1.1e-11
        assert float((dist - dist.round()).abs().max()) < 2e-11 and {0.0, 15.0} < set(dist.round().unique().tolist())
    elif family == "pair":
        assert float(((dist - 0.5) - (dist - 0.5).round()).abs().max()) < 1e-10 and {0.5, 14.5} < set((dist * 2).round().div(2).unique().tolist())
    elif family == "flat":
        assert float((dist - 7.5).abs().max()) < 1e-12
        assert {0.0, 10.0, -20.0} == set(box.amax(2).unique().tolist())  # all zero, and all at a large common value
    elif family == "bump":
        assert float(dist.min()) < 1.0 and float(dist.max()) > 14.0 and len((dist * 64).round().unique()) > 200
    elif family == "bin0":
        assert float(wh.abs().max()) < 1e-10  # a zero-size box
    elif family == "bin15":
        assert float((wh - 30.0).abs().max()) < 1e-9  # a 30-cell box
    else:
        assert float((dist - dist.round()).abs().min()) < 1e-11 and float(((dist * 2) % 2 - 1).abs().min()) < 1e-10 and float((dist - 7.5).abs().min()) < 1e-12


@pytest.mark.parametrize("name", sorted(ALL))
def test_ties_are_exact_and_of_every_kind(name):
    c = ALL[name]
    sc = U.reference(c)[:, 4:]
    best, j = U.first_argmax(sc)
    kind = torch.from_numpy(np.concatenate(c.kind, 1))
    tied_with = lambda s: torch.stack([sc[:, k] == best for k in s]).all(0) & ((sc == best.unsqueeze(1)).sum(1) == len(s))  # noqa: E731
    if c.nc == 1:
        return
    for s in U.tie_sets(min(c.nc, 80)):
        rows = tied_with(s) & (kind == U.ROW_KINDS.index("tie"))
        assert int(rows.sum()) > 0 or c.anchors < 100 * len(U.tie_sets(min(c.nc, 80))), (name, s)
        assert bool((j[rows] == min(s)).all())
    M = U.masked_class(c.nc)
    mt = kind == U.ROW_KINDS.index("masked_tie")
    first_masked, second_masked = mt & tied_with((M, M + 1)), mt & tied_with((M - 1, M))
    assert int(first_masked.sum()) > 0 and int(second_masked.sum()) > 0
    assert bool((j[first_masked] == M).all()) and bool((j[second_masked] == M - 1).all())
    # every row is an exact tie or has a clear winner: no near-tie that a rounding could turn
    top2 = sc.topk(2, 1).values
    assert bool(((top2[:, 0] == top2[:, 1]) | (top2[:, 0] - top2[:, 1] > 1e-3 * top2[:, 0])).all())


@pytest.mark.parametrize("sweep", sorted(SWEEPS))
def test_candidate_bands(sweep):
    cases = SWEEPS[sweep]()
    for c in cases:
        m = U.case_bars(c, cases)["sc"]
        assert 0.0 < m < 1e-5, (c.name, m)  # 8 x an fp32 sigmoid's error
        for conf in U.CONFS:
            for mask in (None, U.class_mask(c.nc)):
                must, may_not, j, tied = U.expected_candidates(c, conf, mask, m)
                band = ~must & ~may_not
                assert band.sum() <= 0.01 * band.size, (c.name, conf, int(band.sum()))
                if c.anchors < 64:
                    continue
                for b in range(U.BATCH):
                    assert must[b].any() and may_not[b].any(), (c.name, conf, b)
            plain, masked = U.expected_candidates(c, conf, None, m)[0], U.expected_candidates(c, conf, U.class_mask(c.nc), m)[0]
            if c.nc > 1:  # (nc 1 has no class to mask)
                assert all((plain[b] & ~masked[b]).any() for b in range(U.BATCH)), (c.name, conf)
        print(f"{sweep} {c.name}: score bar {m:.3e}")
