"""GPU: dy_augment_u8_nchw against the reference's own mosaic canvases (byte for byte, where the arithmetic is exact) and against a
float64 restatement written here; the augmenting loader; training through the graphed step with ``device_augment``."""
import numpy as np
import pytest
import torch

from drone_yolo_amd.data import augment as A
from tests._util import golden

pytestmark = pytest.mark.gpu

G = golden("train_aug.npz")
S0 = int(G["S"])
FL, FU, HOFF = A._lib.DY_AUG_FLIPLR, A._lib.DY_AUG_FLIPUD, A._lib.DY_AUG_HSV_OFF


# ---- the restatement (numpy; ``dt`` = float64 for the yardstick, float32 to measure what rounding alone moves) ------------------------
def hsv_restated(rgb, off, dt):
    """(..., 3) integer-valued RGB -> RandomHSV: H in [0, 180), S, V in [0, 255] rounded; the three look-up rules; back, rounded."""
    rgb = rgb.astype(dt)
    off = np.asarray(off, dtype=np.float32).astype(dt)  # the table stores float32 offsets
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    vmax, vmin = rgb.max(-1), rgb.min(-1)
    d = vmax - vmin
    dd = np.where(d > 0, d, dt(1))
    # (numerators are exact integers and each ratio is ONE division, so a tie in exact arithmetic is a tie here, in either precision)
    num = np.where(vmax == r, dt(30) * (g - b), np.where(vmax == g, dt(30) * (b - r) + dt(60) * d, dt(30) * (r - g) + dt(120) * d))
    num = np.where(num < 0, num + dt(180) * d, num)
    h = np.rint(num / dd)
    h = np.where(h >= 180, h - dt(180), h)
    h = np.where(d > 0, h, dt(0))
    sat = np.where(d > 0, np.rint(dt(255) * d / np.where(vmax > 0, vmax, dt(1))), dt(0))
    h2 = np.trunc(np.mod(h + off[0], dt(180)))
    h2 = np.where(h2 >= 180, dt(0), h2)
    s2 = np.where(sat > 0, np.trunc(np.clip(sat + off[1], 0, 255)), dt(0))
    v2 = np.trunc(np.clip(vmax + off[2], 0, 255))
    i = h2.astype(np.int64) // 30
    f = (h2 - dt(30) * i.astype(dt)) / dt(30)
    s = s2 / dt(255)
    p, q, t = v2 * (1 - s), v2 * (1 - s * f), v2 * (1 - s * (1 - f))
    ro = np.choose(i, [v2, q, p, p, t, v2])
    go = np.choose(i, [t, v2, v2, q, p, p])
    bo = np.choose(i, [p, p, t, v2, v2, q])
    return np.clip(np.rint(np.stack((ro, go, bo), -1)), 0, 255)


def canvas_restated(src, row):
    """The ch x cw canvas of one table row (HWC uint8): 114, then each rectangle pasted in order; a source index outside the tensor
    (or pixels outside its images) shows 114."""
    n, _, hs, ws = src.shape
    c = np.full((int(row["ch"]), int(row["cw"]), 3), 114, dtype=np.uint8)
    for k in range(int(row["n_src"]) if int(row["n_src"]) in (1, 4) else 0):
        i, x1a, y1a, x2a, y2a, x1b, y1b, _ = (int(v) for v in row["src"][k])
        x2a, y2a = min(x2a, c.shape[1]), min(y2a, c.shape[0])
        if x2a <= x1a or y2a <= y1a:
            continue
        patch = np.full((y2a - y1a, x2a - x1a, 3), 114, dtype=np.uint8)
        if 0 <= i < n:
            ys, xs = np.arange(y1b, y1b + y2a - y1a), np.arange(x1b, x1b + x2a - x1a)
            ok = ((ys >= 0) & (ys < hs))[:, None] & ((xs >= 0) & (xs < ws))[None, :]
            got = src[i][:, np.clip(ys, 0, hs - 1)[:, None], np.clip(xs, 0, ws - 1)[None, :]].transpose(1, 2, 0)
            patch = np.where(ok[..., None], got, patch)
        c[y1a:y2a, x1a:x2a] = patch
    return c


def restate(src, table, s, dt=np.float64):
    """(B, 3, s, s) uint8: per output pixel undo the flips, inverse-map with the perspective divide, four bilinear neighbours on the
    canvas (114 outside it), blend, round to nearest, HSV."""
    out = np.empty((len(table), 3, s, s), dtype=np.uint8)
    oy, ox = np.meshgrid(np.arange(s), np.arange(s), indexing="ij")
    for j, row in enumerate(table):
        flags = int(row["flags"])
        x = (s - 1 - ox if flags & FL else ox).astype(dt)
        y = (s - 1 - oy if flags & FU else oy).astype(dt)
        m = row["minv"].astype(dt)
        w = m[6] * x + m[7] * y + m[8]
        u, v = (m[0] * x + m[1] * y + m[2]) / w, (m[3] * x + m[4] * y + m[5]) / w
        ch, cw = int(row["ch"]), int(row["cw"])
        inside = (u > -1) & (v > -1) & (u < cw) & (v < ch)
        u, v = np.where(inside, u, dt(0)), np.where(inside, v, dt(0))
        fu, fv = np.floor(u), np.floor(v)
        ax, ay = (u - fu)[..., None], (v - fv)[..., None]
        cx, cy = fu.astype(np.int64) + 1, fv.astype(np.int64) + 1  # (+1: the canvas below carries a border of 114 one pixel wide)
        c = np.full((ch + 2, cw + 2, 3), 114, dtype=dt)
        c[1:-1, 1:-1] = canvas_restated(src, row)
        v00, v01, v10, v11 = c[cy, cx], c[cy, cx + 1], c[cy + 1, cx], c[cy + 1, cx + 1]
        top, bot = v00 + ax * (v01 - v00), v10 + ax * (v11 - v10)
        px = np.where(inside[..., None], np.rint(top + ay * (bot - top)), dt(114))
        if not flags & HOFF:
            px = hsv_restated(px, row["hsv"], dt)
        out[j] = px.astype(np.uint8).transpose(2, 0, 1)
    return out


def run_kernel(src, table, s, device):
    out = A.launch_augment(torch.from_numpy(src).to(device), table, s)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def fixture_sources():
    """The fixture's images of different shapes as one (N, 3, 64, 64) tensor (each at the top left; 7 elsewhere, which nothing may read)."""
    n = int(G["n_img"])
    src = np.full((n, 3, S0, S0), 7, dtype=np.uint8)
    for i in range(n):
        im = G[f"img_{i}"]
        src[i, :, : im.shape[0], : im.shape[1]] = im.transpose(2, 0, 1)
    return src


def mosaic_row(row, k, minv, flags=HOFF, hsv=(0, 0, 0)):
    ids = [int(v) for v in G[f"mos{k}_ids"]]
    yc, xc = (int(v) for v in G[f"mos{k}_center"])
    a, b, _ = A.mosaic_placement(S0, yc, xc, [G[f"img_{i}"].shape[:2] for i in ids])
    row["n_src"], row["ch"], row["cw"], row["flags"] = 4, 2 * S0, 2 * S0, flags
    for j, i in enumerate(ids):
        row["src"][j] = (i, *a[j], b[j][0], b[j][1], 0)
    row["minv"], row["hsv"] = minv, hsv


def shift(dx, dy):
    return np.array([1, 0, dx, 0, 1, dy, 0, 0, 1], dtype=np.float32)


SHIFTS = [(S0 // 2, S0 // 2), (17, 40), (0, 0), (S0, S0), (-10, 100)]  # the last one leaves the canvas on two sides


def test_exact_case_equals_the_reference_canvas(device):
    """M a pure integer translation at scale 1, HSV off: the output IS the S x S crop of the reference's _mosaic4 canvas, byte for byte,
    for every recorded centre (grey borders and sources smaller than S included); flipped, the flipped crop."""
    src = fixture_sources()
    nm = int(G["n_mosaic"])
    for flags, flip in ((HOFF, lambda c: c), (HOFF | FL, lambda c: c[:, ::-1]), (HOFF | FU, lambda c: c[::-1]), (HOFF | FL | FU, lambda c: c[::-1, ::-1])):
        table = np.zeros(nm * len(SHIFTS), dtype=A.AUG_ROW_DTYPE)
        exp = []
        for k in range(nm):
            big = np.full((4 * S0, 4 * S0, 3), 114, dtype=np.uint8)  # the reference's canvas with borderValue around it
            big[S0 : 3 * S0, S0 : 3 * S0] = G[f"mos{k}_canvas"]
            for t, (dx, dy) in enumerate(SHIFTS):
                mosaic_row(table[k * len(SHIFTS) + t], k, shift(dx, dy), flags)
                exp.append(flip(big[S0 + dy : 2 * S0 + dy, S0 + dx : 2 * S0 + dx]).transpose(2, 0, 1))
        got = run_kernel(src, table, S0, device)
        assert np.array_equal(got, np.stack(exp)), f"flags {flags}"
    # the matrix the reference itself returns for such a shift (fixture), through inverse_matrix
    row = np.zeros(1, dtype=A.AUG_ROW_DTYPE)
    mosaic_row(row[0], 0, A.inverse_matrix(G["persp_m_shift_17_40_M"]))
    assert np.array_equal(run_kernel(src, row, S0, device)[0], G["mos0_canvas"][40 : 40 + S0, 17 : 17 + S0].transpose(2, 0, 1))


def general_case(s, n_src, seed, hsv=False):
    """Sources (random images and smooth ramps) and a table of matrices: scale 0.5 to 1.5, rotation, shear, a perspective term."""
    g = np.random.default_rng(seed)
    n = 6
    src = g.integers(0, 256, (n, 3, s, s), dtype=np.uint8)
    yy, xx = np.meshgrid(np.arange(s), np.arange(s), indexing="ij")
    src[1] = np.stack(((xx * 255 // (s - 1)), (yy * 255 // (s - 1)), ((xx + yy) * 255 // (2 * s - 2)))).astype(np.uint8)
    src[4] = np.stack((255 - (yy * 255 // (s - 1)), (xx * yy * 255 // ((s - 1) ** 2)), np.full((s, s), 90))).astype(np.uint8)
    params = [(0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.5, 0.5), (0.0, 0.5, 0.0, 0.0, 0.0, 0.0, 0.53, 0.47), (0.0, 1.5, 0.0, 0.0, 0.0, 0.0, 0.45, 0.55),
              (12.0, 1.2, 0.0, 0.0, 0.0, 0.0, 0.5, 0.52), (-7.0, 0.8, 6.0, -4.0, 0.0, 0.0, 0.58, 0.41), (3.0, 1.1, 2.0, 1.0, 0.0004, -0.0002, 0.5, 0.5),
              (0.0, 0.731, 0.0, 0.0, 0.0, 0.0, 0.4123, 0.5871), (-15.0, 1.37, -3.0, 5.0, -0.0003, 0.0005, 0.44, 0.56)]
    for _ in range(0 if s > 64 else 248):  # small outputs: many more rows, so that the shares below are counts of hundreds of bytes, not of four
        pp = g.uniform(-0.0005, 0.0005, 2) * (g.random() < 0.5)
        params.append((g.uniform(-15, 15), g.uniform(0.5, 1.5), g.uniform(-5, 5), g.uniform(-5, 5), pp[0], pp[1], g.uniform(0.4, 0.6), g.uniform(0.4, 0.6)))
    table = np.zeros(len(params), dtype=A.AUG_ROW_DTYPE)
    for j, (ang, sc, shx, shy, px, py, tx, ty) in enumerate(params):
        row = table[j]
        canvas = (2 * s, 2 * s) if n_src == 4 else (s, s)
        if n_src == 4:
            yc, xc = (int(g.uniform(s / 2, 3 * s / 2)) for _ in range(2))
            hw = [(int(g.integers(s // 2, s + 1)), int(g.integers(s // 2, s + 1))) for _ in range(4)]
            a, b, _ = A.mosaic_placement(s, yc, xc, hw)
            for k in range(4):
                row["src"][k] = (int(g.integers(0, n)), *a[k], b[k][0], b[k][1], 0)
        else:
            a1, b1, _ = A.center_placement(s, (int(g.integers(s // 2, s + 1)), s))
            row["src"][0] = (j % n, *a1, b1[0], b1[1], 0)
        row["n_src"], row["ch"], row["cw"] = n_src, canvas[0], canvas[1]
        row["flags"] = HOFF | (FL if j % 3 == 1 else 0) | (FU if j % 4 == 2 else 0)
        row["minv"] = A.inverse_matrix(A.affine_matrix(canvas, (s, s), ang, sc, shx, shy, px, py, tx, ty))
        if hsv:  # RandomHSV's range at gains (0.5, 0.9, 0.9); fractions of .05 / .15 / ..: x + r never lies within round-off of an integer
            row["hsv"] = np.floor(g.uniform(-1, 1, 3) * (90, 229, 229) * 10) / 10 + 0.05
    return src, table


@pytest.mark.parametrize("s,n_src", [(64, 1), (64, 4), (640, 1), (640, 4)])
def test_general_case_against_the_restatement(s, n_src, device):
    """Every byte within 1 level of the float64 restatement.  The share of bytes that differ at all is rounding noise (a blend that lands
    within fp32 round-off of x.5); its size is measured here as the share that differs between a float32 and a float64 run of the
    restatement on these very inputs, and the kernel's share may be at most 3 times that (the kernel contracts multiply-adds and divides
    in another order than numpy's float32, so it is a second float32 evaluation, not the same one).  Measured on an MI355X, share of the
    float32 restatement / of the kernel: S = 64, n_src 1: 6.39e-5 / 5.98e-5; S = 64, n_src 4: 1.35e-4 / 1.31e-4; S = 640, n_src 1:
    3.73e-4 / 3.58e-4; S = 640, n_src 4: 5.79e-4 / 5.69e-4; max |difference| = 1 level in all four.  HSV is off in this case: one differing level in front
    of the hue quantisation is not bounded by one level behind it, so the colour path is checked on exact inputs (identity matrix) below."""
    src, table = general_case(s, n_src, seed=100 + s + n_src)
    ref = restate(src, table, s, np.float64).astype(np.int16)
    r32 = restate(src, table, s, np.float32).astype(np.int16)
    got = run_kernel(src, table, s, device).astype(np.int16)
    share32, share = float((r32 != ref).mean()), float((got != ref).mean())
    worst = int(np.abs(got - ref).max())
    print(f"augment general case S={s} n_src={n_src}: max |kernel - f64| = {worst}, share differing: float32 restatement {share32:.3e}, kernel {share:.3e}")
    assert (ref != 114).mean() > 0.3  # (the case is not mostly border)
    assert worst <= 1
    assert share <= 3 * share32, (share, share32)


@pytest.mark.parametrize("s,n_src", [(64, 1), (64, 4), (640, 1), (640, 4)])
def test_general_case_with_hsv(s, n_src, device):
    """Warp and HSV in ONE launch, the combination every training row uses (blended pixels, the 114 border and fill, flips, n_src 1
    and 4).  A one-level difference of the blend in front of the hue quantisation is not bounded by one level behind it, so the yardstick
    is the float64 HSV restatement applied to what the kernel itself blends: kernel(HSV on) within 1 level of
    hsv_restated(kernel(HSV off), the row's offsets), every byte.  The blend itself is held to the restatement by the test above; the
    two together cover the issue's general case.  Where the float64 restatement of the whole path blends the same bytes as the kernel,
    it must then agree within 1 level too (asserted on exactly those pixels)."""
    src, table = general_case(s, n_src, seed=100 + s + n_src, hsv=True)
    plain = table.copy()
    table["flags"] &= ~HOFF
    off = run_kernel(src, plain, s, device)
    got = run_kernel(src, table, s, device).astype(np.int16)
    exp = np.stack([hsv_restated(off[j].transpose(1, 2, 0), table[j]["hsv"], np.float64).transpose(2, 0, 1) for j in range(len(table))]).astype(np.int16)
    worst, share = int(np.abs(got - exp).max()), float((got != exp).mean())
    print(f"augment warp + HSV S={s} n_src={n_src}: max |kernel - hsv_f64(kernel blend)| = {worst}, share differing {share:.3e}, changed by HSV {(got != off).mean():.2f}")
    assert (got != off).mean() > 0.5  # (HSV did act)
    assert worst <= 1
    ref_off = restate(src, plain, s, np.float64)
    ref = restate(src, table, s, np.float64).astype(np.int16)
    same = (ref_off == off).all(1, keepdims=True).repeat(3, 1)  # pixels whose three blended bytes agree
    assert same.mean() > 0.99 and int(np.abs(got - ref)[same].max()) <= 1


def test_hsv_restatement_against_colorsys():
    """The HSV yardstick anchored outside the code it judges.  (a) Zero offsets are nearly the identity: H is quantised to 1/180 of the
    circle = half a quantum of 1 degree of a 60-degree sector, i.e. at most V S / 60 <= 4.25 levels, S to 1/255 (<= 0.5 level), plus the
    final rounding: <= 5 levels.  (b) With offsets, the same rule written with the standard library's colorsys (float HSV, quantised to
    the 8-bit ranges, the three look-up rules, back) agrees within 1 level wherever colorsys' float quotients quantise H and S to the same
    integers, which is nearly everywhere (they differ only at exact ties, computed inexactly there), and nowhere by more than one further
    hue quantum (4.25 + 1 -> 6 levels, rounded up to 7 for the two roundings)."""
    import colorsys

    g = np.random.default_rng(11)
    rgb = g.integers(0, 256, (20000, 3))
    rgb[:2000] = rgb[:2000, :1]  # greys
    back = hsv_restated(rgb, (0.0, 0.0, 0.0), np.float64)
    assert np.abs(back - rgb).max() <= 5 and np.array_equal(back[:2000], rgb[:2000])
    off = np.array([20.05, 30.25, -40.5], dtype=np.float32).astype(np.float64)
    exp = np.empty_like(rgb)
    for k, (r, gg, b) in enumerate(rgb.tolist()):
        h, s, v = colorsys.rgb_to_hsv(r / 255, gg / 255, b / 255)
        hq, sq, vq = np.rint(h * 180) % 180, np.rint(s * 255), np.rint(v * 255)
        h2 = np.trunc((hq + off[0]) % 180) % 180
        s2 = np.trunc(np.clip(sq + off[1], 0, 255)) if sq > 0 else 0.0
        v2 = np.trunc(np.clip(vq + off[2], 0, 255))
        exp[k] = np.rint(np.array(colorsys.hsv_to_rgb(h2 / 180, s2 / 255, v2 / 255)) * 255)
    got = hsv_restated(rgb, off, np.float64)
    diff = np.abs(got - exp)
    print(f"hsv restatement vs colorsys: max {diff.max()}, share beyond one level {(diff > 1).mean():.3e}")
    assert diff.max() <= 7 and (diff > 1).mean() < 0.01


def test_hsv_alone_and_greys(device):
    """Identity matrix (the blend is exact), HSV on: within 1 level of the float64 restatement; grey pixels (S = 0) stay grey whatever the
    offsets, as the reference's ``lut_sat[0] = 0`` intends."""
    s = 64
    g = np.random.default_rng(5)
    src = g.integers(0, 256, (4, 3, s, s), dtype=np.uint8)
    src[1] = np.repeat(g.integers(0, 256, (1, s, s), dtype=np.uint8), 3, 0)  # greys
    src[2, :, :, : s // 2] = src[2, :1, :, : s // 2]  # half grey
    src[3] = (np.arange(s * s * 3).reshape(3, s, s) * 7 % 256).astype(np.uint8)
    offs = [(0.0, 0.0, 0.0), (2.7, 178.5, 102.0), (-2.7, -120.25, -60.5), (1.3, 40.75, -101.3), (-0.6, 254.0, 254.0), (95.4, -254.0, 10.2)]
    table = np.zeros(len(offs) * 4, dtype=A.AUG_ROW_DTYPE)
    for j in range(len(table)):
        row = table[j]
        row["n_src"], row["ch"], row["cw"], row["flags"] = 1, s, s, 0
        row["src"][0] = (j % 4, 0, 0, s, s, 0, 0, 0)
        row["minv"], row["hsv"] = shift(0, 0), offs[j // 4]
    got = run_kernel(src, table, s, device).astype(np.int16)
    ref = restate(src, table, s, np.float64).astype(np.int16)
    worst, share = int(np.abs(got - ref).max()), float((got != ref).mean())
    print(f"augment HSV alone: max |kernel - f64| = {worst}, share differing {share:.3e}")
    assert worst <= 1
    for j in range(len(table)):
        grey = (src[j % 4][0] == src[j % 4][1]) & (src[j % 4][1] == src[j % 4][2])
        o = got[j]
        assert (o[0][grey] == o[1][grey]).all() and (o[1][grey] == o[2][grey]).all(), f"row {j}: a grey pixel took a colour"
        v2 = np.trunc(np.clip(src[j % 4][0][grey].astype(np.float64) + np.float32(offs[j // 4][2]), 0, 255))
        assert np.array_equal(o[0][grey], v2.astype(np.int16))


def test_out_of_range_source_gives_grey_and_spares_the_rest(device):
    """A bounds rule, checked with a valid launch: a row whose source index lies outside [0, N), or whose n_src is neither 1 nor 4, reads
    nothing and shows 114 there; the other rectangles and the other rows are as they should be."""
    src = fixture_sources()
    table = np.zeros(4, dtype=A.AUG_ROW_DTYPE)
    ks = [1, 0, 2, 3]  # (row 1, the one with the bad indices, is mosaic 0: its centre is the centre of the crop)
    for j, k in enumerate(ks):
        mosaic_row(table[j], k, shift(S0 // 2, S0 // 2))
    table[1]["src"][1][0] = len(src) + 5
    table[1]["src"][2][0] = -1
    table[2]["n_src"] = 3
    table[3]["src"][0][5] = 10_000  # a source origin far outside the image
    got = run_kernel(src, table, S0, device)
    crop = lambda k: G[f"mos{k}_canvas"][S0 // 2 : S0 // 2 + S0, S0 // 2 : S0 // 2 + S0].transpose(2, 0, 1)  # noqa: E731
    assert np.array_equal(got[0], crop(1))
    assert np.array_equal(got, restate(src, table, S0))
    assert (got[2] == 114).all()
    yc, xc = (int(v) - S0 // 2 for v in G["mos0_center"])
    assert (yc, xc) == (S0 // 2, S0 // 2)
    assert np.array_equal(got[1][:, :yc, :xc], crop(0)[:, :yc, :xc]) and np.array_equal(got[1][:, yc:, xc:], crop(0)[:, yc:, xc:])  # quadrants 0 and 3 intact
    assert (got[1][:, :yc, xc:] == 114).all() and (got[1][:, yc:, :xc] == 114).all()
    yc, xc = (int(v) - S0 // 2 for v in G["mos3_center"])
    assert (got[3][:, :yc, :xc] == 114).all() and np.array_equal(got[3][:, yc:, xc:], crop(3)[:, yc:, xc:])


# ---- loader and trainer ---------------------------------------------------------------------------------------------------------------
def test_loader_batches(device):
    from drone_yolo_amd.engine.trainer import AugmentLoader, get_cfg, synthetic_dataset

    s = 64
    data = synthetic_dataset(24, s, seed=1005, nc=10)
    args = get_cfg(dict(device_augment=True, degrees=5.0, shear=2.0, flipud=0.2))

    def batches(resident, seed=3):
        ld = AugmentLoader(data, 8, args, s, device, epochs=20, seed=seed, resident=resident)
        ld.set_epoch(1)
        out = [(b["img"].cpu().numpy(), b["batch_idx"].numpy(), b["cls"].numpy(), b["bboxes"].numpy(), ld.last_table.copy()) for b in ld]
        assert ld.resident == resident
        return out

    a, b, c = batches(True), batches(True), batches(False)
    assert len(a) == 3
    for (img, bi, cls, box, table), rb, rc in zip(a, b, c):
        assert img.dtype == np.uint8 and img.shape == (8, 3, s, s) and box.dtype == np.float32 and cls.shape == (len(bi), 1)
        assert box.min() >= 0.0 and box.max() <= 1.0 and len(bi) > 0 and bi.max() <= 7
        wh = box[:, 2:] * s  # what box_candidates asks of a kept box: more than 2 pixels each way, aspect ratio under 100
        assert (wh > 2 - 1e-3).all() and (np.maximum(wh[:, 0] / wh[:, 1], wh[:, 1] / wh[:, 0]) < 100).all()
        assert (table["n_src"] == 4).all() and (img != 114).mean() > 0.3
        for x, y in zip((img, bi, cls, box), rb):
            assert np.array_equal(x, y)  # two loaders, one seed
        for x, y in zip((img, bi, cls, box), rc):
            assert np.array_equal(x, y)  # resident dataset and per-batch upload
        assert table["src"][:, :, 0].max() < 24 and rc[4]["src"][:, :, 0].max() < 32  # (the upload mode's indices are positions in the upload)
    other = batches(True, seed=4)
    assert not np.array_equal(other[0][0], a[0][0])
    auto = AugmentLoader(data, 8, args, s, device, epochs=20, seed=3)
    assert auto.resident and auto.label_capacity() % 64 == 0 and auto.label_capacity() >= 128
    late = AugmentLoader(data, 8, get_cfg(dict(device_augment=True, close_mosaic=2)), s, device, epochs=5, seed=3)
    seen = []
    for ep in range(5):
        late.set_epoch(ep)
        next(iter(late))
        seen.append(sorted(set(late.last_table["n_src"].tolist())))
    assert seen == [[4], [4], [4], [1], [1]]


def test_training_with_device_augment(device, tmp_path):
    """A few epochs of DetectionTrainer.train() on synthetic:64 with device_augment: the graphed step runs (finite losses), ONE capture
    for the training shape although the label counts of mosaics wander (the capacity is seeded from the loader's bound), the loader writes
    into the step's resident batch, and close_mosaic switches the four-image branch off at epoch epochs - close_mosaic."""
    from drone_yolo_amd.engine.trainer import AugmentLoader, DetectionTrainer

    seen = {}

    class Watch(DetectionTrainer):
        def train_batch(self, batch, ni, epoch, nb):
            seen.setdefault(epoch, []).append((sorted(set(self.train_loader.last_table["n_src"].tolist())), len(self.__dict__.get("_graphs", {})),
                                               self.static_image() is not None and batch["img"].data_ptr() == self.static_image().data_ptr()))
            out = super().train_batch(batch, ni, epoch, nb)
            assert bool(torch.isfinite(out[0]).all())
            return out

    t = Watch(overrides=dict(model="yolov8n-p2-repvgg.yaml", nc=10, data="synthetic:64", epochs=4, close_mosaic=2, imgsz=64, batch=16, nbs=16, device=0,
                             dtype="bf16", optimizer="SGD", lr0=0.01, warmup_epochs=0.0, project=str(tmp_path), name="aug", val=False, device_augment=True))
    out = t.train()
    assert isinstance(t.train_loader, AugmentLoader) and t.train_loader.resident
    assert all(np.isfinite(v) for k, v in out.items() if k.startswith("train/"))
    assert [sorted({tuple(n) for n, _, _ in seen[e]}) for e in range(4)] == [[(4,)], [(4,)], [(1,)], [(1,)]]
    graphs = t.__dict__["_graphs"]
    assert len(graphs) == 1 and next(iter(graphs))[0] == (16, 3, 64, 64), list(graphs)  # one capture for the training shape
    assert max(g for e in seen.values() for _, g, _ in e) == 1
    assert next(iter(graphs))[3] == t.train_loader.label_capacity()
    assert all(w for _, _, w in seen[3])  # by the last epoch every batch was written straight into static_image()


def test_keys_absent_training_is_bitwise_the_parent(device, tmp_path):
    """With the new keys absent the loop computes what it computed before the feature: the per-epoch mean loss items of a three-epoch
    bf16 run equal, bit for bit, those recorded from the PARENT commit on an MI355X into tests/golden/train_aug_parent.npz (float32 bit
    patterns); device_augment=False with augmentation arguments set takes the same path and gives the same bits."""
    from drone_yolo_amd.engine.trainer import DetectionTrainer, TensorLoader

    ref = golden("train_aug_parent.npz")["loss_items"]
    common = dict(model="yolov8n-p2-repvgg.yaml", nc=10, data="synthetic:32", epochs=3, imgsz=64, batch=8, nbs=8, device=0, dtype="bf16", optimizer="SGD", lr0=0.01,
                  warmup_epochs=1.0, project=str(tmp_path), val=False, seed=0)
    for name, extra in (("absent", {}), ("off", dict(device_augment=False, mosaic=0.3, fliplr=0.0, hsv_h=0.5))):
        rows = []

        class Rec(DetectionTrainer):
            def save_metrics(self, metrics):
                rows.append(self.tloss.detach().float().cpu().numpy().copy())
                super().save_metrics(metrics)

        t = Rec(overrides=dict(common, name=name, **extra))
        t.train()
        assert type(t.train_loader) is TensorLoader
        got = np.stack(rows).astype(np.float32)
        assert got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (name, got, ref)


def test_training_on_a_dataset_yaml_with_device_augment(device, tmp_path):
    """The public path end to end: a YOLO-format folder written here -> DetectionTrainer(data=<yaml>, device_augment=True) -> one epoch
    through the augmenting loader (the mosaic pastes the ``rect`` regions of images of different shapes) and a validation pass on the
    ``val`` split, which is never augmented."""
    import csv

    from drone_yolo_amd.engine.trainer import AugmentLoader, DetectionTrainer, TensorLoader
    from tests.test_augment_host import write_yolo_folder

    shapes = {"train": [(48, 64), (64, 40), (100, 80), (64, 64), (30, 60), (64, 50), (50, 64), (64, 64)], "val": [(64, 48), (40, 64), (64, 64), (90, 120)]}
    path = write_yolo_folder(tmp_path / "set", shapes)
    t = DetectionTrainer(overrides=dict(model="yolov8n-p2-repvgg.yaml", nc=4, data=path, epochs=1, imgsz=64, batch=4, nbs=4, device=0, dtype="bf16", optimizer="SGD",
                                        lr0=0.01, warmup_epochs=0.0, project=str(tmp_path), name="y", device_augment=True, close_mosaic=0))
    out = t.train()
    ld = t.train_loader
    assert isinstance(ld, AugmentLoader) and type(t.val_loader) is TensorLoader and t.val_loader.n == 4
    assert ld.aug.rect.tolist()[:3] == [[8, 0, 48, 64], [0, 12, 64, 40], [0, 6, 64, 52]]  # (top, left, h, w); the third image resized to 64 x 52
    tb = ld.last_table
    assert (tb["n_src"] == 4).all()
    for row in tb:  # every pasted rectangle starts inside its image's valid region and is no larger than it
        for i, x1a, y1a, x2a, y2a, x1b, y1b, _ in row["src"].tolist():
            top, left, h, w = ld.aug.rect[i].tolist()
            assert left <= x1b and top <= y1b and x1b + (x2a - x1a) <= left + w and y1b + (y2a - y1a) <= top + h
    assert all(np.isfinite(v) for k, v in out.items() if k.startswith("train/"))
    rows = list(csv.DictReader(open(tmp_path / "y" / "results.csv")))
    assert len(rows) == 1 and "metrics/mAP50(B)" in rows[0] and np.isfinite(float(rows[0]["val/cls_loss"]))
