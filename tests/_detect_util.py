"""The Detect decode sweep (tests/test_detect_geometry_host.py, tests/test_detect_geometry_gpu.py): logit families a trained head
produces, built so that the fp32 logits that reach the decode row are known EXACTLY on every path, and a float64 restatement of
the decode to hold the kernels to.  Not collected; needs no GPU.

One construction serves every path.  A logit is ``L = S * x + bias`` with ``S = 0.5``, ``bias = B0 = -20`` and ``x`` in
``{0} U [20, 60]`` on the bfloat16 grid (so float16 and fp32 hold it too): ``L`` in ``{-20} U [-10, 10]``, one exact product plus
a bias, exact in fp32.
  * dy_detect_decode takes ``L`` itself;
  * dy_detect_head_decode (f32 / bf16 / f16 / split float16) takes ``x`` behind 1x1 weights ``S * identity`` (box) and
    ``S * selector`` (class: class c reads channel c % 80, classes 80.. get the bias B0 - 32: a second, far background);
  * dy_detect_branch_fused (conv3x3_hhead) takes ``x`` behind a centre-tap identity 3x3 + SiLU, which rounds back to ``x`` in both
    16-bit types for every ``x`` used (``silu_round_trip``: 1 - sigmoid(20) = 2e-9), and the same 1x1.
``wide_case`` (dy_detect_decode only: it takes any fp32 logit) adds spreads of +-60, where exp2 underflows.

Bars (``case_bars``; not constants chosen here): per case and output group (xy, wh, scores) 8 x the largest difference between the oracle's
decode in fp32 (oracle.drone_yolo_oracle.detect_decode, CPU) and ``ref_decode`` in float64 on the same logits; boxes absolute, scores
relative to max(score, 1e-7).  A bar of 0 (the fp32 run exact) becomes the largest bar of the family's cases.
"""
import functools

import numpy as np
import torch

from oracle import drone_yolo_oracle as O

BATCH = 2
LEVELS = [(23, 25), (9, 17), (5, 7), (1, 1)]  # 575 anchors: nine 64-anchor tiles, the last ragged; 9x17: ragged against the 8x16 tile both ways
STRIDES = [4.0, 8.0, 16.0, 32.0]
P2ROW = ([(2, 384)], [4.0])  # gx comes from the level's width in every kernel: two rows of the 1536-px P2 grid, gx up to 383 at stride 4
S, B0 = 0.5, -20.0
FAR = 32.0  # classes 80.. sit this far below the channel they share
FAMILIES = ("peak", "pair", "flat", "bump", "bin0", "bin15", "mixed")
CONFS = (0.25, 0.001)
ROW_KINDS = ("background", "low", "positive", "near25", "near001", "tie", "masked_tie", "masked_pos")
FACTOR = 8.0  # tests/test_obb_gpu.py::_theta_tol


def masked_class(nc):
    """The class the mask removes: 3 (the last of lane quarter 0 in conv3x3_hhead), 1 for nc 3; none for nc 1."""
    return None if nc == 1 else min(3, nc - 2)


def class_mask(nc):
    m = torch.ones(nc, dtype=torch.uint8)
    if masked_class(nc) is not None:
        m[masked_class(nc)] = 0
    return m


def snap(L):
    """Ideal logits (float64 array) -> (x, L'): the storage value of each and the logit it stands for, L' = S x + B0 exactly."""
    x = 2.0 * (np.asarray(L, np.float64) - B0)
    xt = torch.from_numpy(np.clip(x, 0.0, 60.0)).to(torch.bfloat16).double().numpy()
    xt = np.where(x < 20.0, 0.0, np.clip(xt, 20.0, 60.0))
    return xt, S * xt + B0


def silu_round_trip(x, dtype):
    """silu(x), in float64, rounded to ``dtype``."""
    t = torch.from_numpy(np.asarray(x, np.float64))
    return (t * torch.sigmoid(t)).to(dtype).double().numpy()


# ---- the families ----
def _peak(rng, n, bins=None):
    i = rng.choice([0, 15, 1, 7, 8, 14], n) if bins is None else np.full(n, bins)
    v = np.full((n, 16), -20.0)
    v[np.arange(n), i] = 10.0
    return v


def _pair(rng, n):
    i = rng.choice([0, 14, 3, 7, 11], n)  # 3|4, 7|8, 11|12: the pair straddles two lane quarters of conv3x3_hhead
    v = np.full((n, 16), -20.0)
    v[np.arange(n), i] = v[np.arange(n), i + 1] = 8.0
    return v


def _flat(rng, n):
    return np.repeat(rng.choice([0.0, 10.0, -20.0], n)[:, None], 16, 1)


def _bump(rng, n):
    t = rng.uniform(0.0, 15.0, n)[:, None]
    tau = rng.choice([0.3, 1.0, 3.0, 10.0, 40.0], n)[:, None]
    return np.maximum(4.0 - (np.arange(16)[None] - t) ** 2 / tau, -10.0)


def dfl_rows(family, rng, n):
    """(n, 4, 16) ideal box logits of ``n`` anchors."""
    if family in ("bin0", "bin15"):
        return _peak(rng, 4 * n, 0 if family == "bin0" else 15).reshape(n, 4, 16)
    if family == "mixed":
        parts = np.stack([f(rng, 4 * n) for f in (_peak, _pair, _flat, _bump)])
        return parts[rng.integers(0, 4, 4 * n), np.arange(4 * n)].reshape(n, 4, 16)
    return {"peak": _peak, "pair": _pair, "flat": _flat, "bump": _bump}[family](rng, 4 * n).reshape(n, 4, 16)


def tie_sets(nc):
    """Class sets of the exact ties: inside a lane quarter, across quarter boundaries (3|4, 0|15), all classes."""
    sets = [(1, 2), (3, 4), (0, 15), (5, 6, 9), tuple(range(nc))]
    return [s for s in sets if max(s) < nc and len(s) > 1]


def cls_rows(rng, n, nc):
    """(n, nc) ideal class logits of the first min(nc, 80) classes and each row's kind (index into ROW_KINDS).  Every 8 consecutive
    anchors hold one row of each kind; ties alternate between a value that clears both confs and one that clears 0.001 only."""
    ncs = min(nc, 80)
    kind = (np.arange(n) + rng.integers(0, 8)) % 8
    v = rng.uniform(-20.0, -8.0, (n, ncs))
    v[rng.random((n, ncs)) < 0.3] = -20.0
    M, ts = masked_class(nc), tie_sets(ncs)
    hot = rng.integers(0, ncs, n)
    if M is not None:
        hot = np.where(hot == M, (M + 1) % ncs, hot)
    val = {1: rng.uniform(-6.5, -2.0, n), 2: rng.uniform(0.0, 8.0, n), 3: -1.0986 + rng.uniform(-0.5, 0.5, n), 4: -6.9068 + rng.uniform(-0.4, 0.4, n)}
    for r in range(n):
        k = kind[r]
        if k in val:
            v[r, hot[r]] = val[k][r]
        elif k == 5 and ts:
            v[r, list(ts[(r // 8) % len(ts)])] = 2.0 if (r // (8 * len(ts))) % 2 == 0 else -3.0
        elif k == 6 and M is not None:
            # even: the masked class ties with a LATER kept one, the first arg-max is masked and the anchor dropped;
            # odd: a kept class ties with the later masked one, and the anchor stays
            v[r, [M, M + 1] if (r // 8) % 2 == 0 else [M - 1, M]] = 3.0
        elif k == 7 and M is not None:
            v[r, M] = 4.0
        elif k >= 5:  # nc 1: no tie and no mask; a plain positive
            v[r, 0] = 1.5
    return v, kind


class Case:
    """name, family, nc, shapes, strides; x: per level (B, 64 + min(nc, 80), h, w) float64 storage values; feats: per level the exact
    logits (B, 64 + nc, h, w) float64; kind: per level (B, h * w) row kinds."""


def class_affine(nc):
    """(source channel, bias) of every class logit: L_c = S x[src_c] + bias_c."""
    c = np.arange(nc)
    return c % 80, B0 - FAR * (c // 80)


@functools.lru_cache(maxsize=None)
def make_case(family, nc, p2row=False):
    shapes, strides = P2ROW if p2row else (LEVELS, STRIDES)
    rng = np.random.default_rng([FAMILIES.index(family), nc, int(p2row)])
    c = Case()
    c.name, c.family, c.nc, c.shapes, c.strides = f"{family}-nc{nc}" + ("-p2row" if p2row else ""), family, nc, shapes, strides
    c.x, c.feats, c.kind = [], [], []
    src, bias = class_affine(nc)
    for h, w in shapes:
        n = BATCH * h * w
        cl, kind = cls_rows(rng, n, nc)
        ideal = np.concatenate([dfl_rows(family, rng, n).reshape(n, 64), cl], 1)
        x, _ = snap(ideal)
        L = np.concatenate([S * x[:, :64] + B0, S * x[:, 64 + src] + bias[None]], 1)
        assert np.array_equal(L.astype(np.float32).astype(np.float64), L)
        to_map = lambda a: torch.from_numpy(np.ascontiguousarray(a.reshape(BATCH, h, w, -1).transpose(0, 3, 1, 2)))  # noqa: E731
        c.x.append(to_map(x)), c.feats.append(to_map(L)), c.kind.append(kind.reshape(BATCH, h * w))
    c.anchors = sum(h * w for h, w in shapes)
    return c


@functools.lru_cache(maxsize=None)
def wide_case(nc):
    """dy_detect_decode only: fp32 logits spread over +-60.  Peaks of +60 over -60 (exp2 of -173 underflows), steep bumps, uniform rows;
    class rows as everywhere, with a background stretched to -60."""
    rng = np.random.default_rng([99, nc])
    c = Case()
    c.name, c.family, c.nc, c.shapes, c.strides, c.x = f"wide-nc{nc}", "wide", nc, LEVELS, STRIDES, None
    c.feats, c.kind = [], []
    for h, w in LEVELS:
        n = BATCH * h * w
        box = np.stack([np.where(_peak(rng, 4 * n) > 0.0, 60.0, -60.0), _bump(rng, 4 * n) * 12.0, rng.uniform(-60.0, 60.0, (4 * n, 16))])
        box = np.clip(box[rng.integers(0, 3, 4 * n), np.arange(4 * n)], -120.0, 60.0).reshape(n, 64)
        cl, kind = cls_rows(rng, n, nc)
        cl = np.where(cl < -8.0, cl * 3.0, cl)
        L = np.concatenate([box, cl], 1).astype(np.float32).astype(np.float64)
        c.feats.append(torch.from_numpy(np.ascontiguousarray(L.reshape(BATCH, h, w, -1).transpose(0, 3, 1, 2))))
        c.kind.append(kind.reshape(BATCH, h * w))
    c.anchors = sum(h * w for h, w in LEVELS)
    return c


# ---- the reference ----
def ref_decode(feats, strides, nc, dtype=torch.float64):
    """The Detect decode restated: softmax expectation over the 16 bins of each side, anchor point (gx + .5, gy + .5), xywh times the
    stride, sigmoid.  feats: per level (B, 64 + nc, h, w) -> (B, 4 + nc, A)."""
    out = []
    bins = torch.arange(16, dtype=dtype)
    for f, s in zip(feats, strides):
        b, _, h, w = f.shape
        f = f.to(dtype).reshape(b, 64 + nc, h * w)
        box = f[:, :64].reshape(b, 4, 16, h * w)
        e = torch.exp(box - box.amax(2, keepdim=True))
        d = (e * bins.view(1, 1, 16, 1)).sum(2) / e.sum(2)
        a = torch.arange(h * w)
        ax, ay = (a % w).to(dtype) + 0.5, (a // w).to(dtype) + 0.5
        x1, y1, x2, y2 = ax - d[:, 0], ay - d[:, 1], ax + d[:, 2], ay + d[:, 3]
        xywh = torch.stack(((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1), 1) * s
        out.append(torch.cat((xywh, 1.0 / (1.0 + torch.exp(-f[:, 64:]))), 1))
    return torch.cat(out, 2)


def first_argmax(sc):
    """(best, class) over dim 1 of (B, nc, A): the LOWEST index among equal maxima."""
    best = sc.amax(1)
    return best, (sc == best.unsqueeze(1)).to(torch.int8).argmax(1)


def errors(y, ref):
    """Max error of (B, 4 + nc, A) ``y`` against float64 ``ref`` per group: xy and wh absolute, scores relative to max(score, 1e-7)."""
    y, ref = y.double(), ref.double()
    d = (y - ref).abs()
    return dict(xy=float(d[:, :2].max()), wh=float(d[:, 2:4].max()), sc=float((d[:, 4:] / ref[:, 4:].clamp_min(1e-7)).max()))


@functools.lru_cache(maxsize=None)
def reference(case):
    return ref_decode(case.feats, case.strides, case.nc)


@functools.lru_cache(maxsize=None)
def _raw_bars(case):
    y32 = O.detect_decode([f.float() for f in case.feats], case.strides, case.nc)
    return {k: FACTOR * v for k, v in errors(y32, reference(case)).items()}


def family_cases(case, cases):
    return [c for c in cases if c.family == case.family]


def case_bars(case, cases):
    """The bars of ``case``; ``cases``: every case of the sweep it belongs to (a bar of 0 takes the family's largest)."""
    bars = dict(_raw_bars(case))
    for k, v in bars.items():
        if v == 0.0:
            bars[k] = max(_raw_bars(c)[k] for c in family_cases(case, cases))
    return bars


def expected_candidates(case, conf, mask, m):
    """From the float64 scores, per image: (must, may_not, cls, tied) boolean / index arrays over the anchors.  must: best above
    conf (1 + m) and the first arg-max class kept by ``mask``; may_not: best below conf (1 - m), or that class masked; anchors in
    neither are the band.  tied: the top two scores are equal (then cls is the lowest tied index)."""
    sc = reference(case)[:, 4:]
    best, j = first_argmax(sc)
    keep = torch.ones_like(best, dtype=torch.bool) if mask is None else mask.bool()[j]
    top2 = sc.topk(min(2, case.nc), 1).values
    tied = top2[:, 0] == top2[:, -1] if case.nc > 1 else torch.zeros_like(keep)
    clear = torch.ones_like(keep) if case.nc == 1 else (tied | ((top2[:, 0] - top2[:, -1]) > m * top2[:, 0]))
    must = (best > conf * (1 + m)) & keep & clear
    may_not = (best < conf * (1 - m)) | (~keep & clear)
    return must.numpy(), may_not.numpy(), j.numpy(), tied.numpy()


# ---- the sweeps of the three entry points ----
def sweep(nc_main, nc_rest, with_p2row=True):
    """Every family at ``nc_main``, the mixed family at each of ``nc_rest`` and on the P2 row."""
    cs = [make_case(f, nc_main) for f in FAMILIES] + [make_case("mixed", nc) for nc in nc_rest]
    return cs + ([make_case("mixed", nc_main, True)] if with_p2row else [])


def decode_cases():
    return sweep(80, (3,)) + [wide_case(3), wide_case(80)]


def head_cases():
    # (40 and 80: class rows that stop short of the weight pack's 64- and 128-row tiles)
    return sweep(10, (1, 40, 80, 128))


def hhead_cases():
    return sweep(10, (1, 16))


def workspace_views(bufs):
    """(counts (N,) int32, keys (N, P) int64, cls (N, A) int16) views of an NmsBuffers workspace (csrc/nms_ws.h)."""
    n, A = bufs.batch, bufs.anchors
    P = 1 << (A - 1).bit_length()
    off = (4 * n + 255) // 256 * 256
    ws = bufs.workspace
    return ws[: 4 * n].view(torch.int32), ws[off : off + n * P * 8].view(torch.int64).view(n, P), ws[off + n * P * 8 : off + n * P * 8 + n * A * 2].view(torch.int16).view(n, A)
