"""The containment harness (tests/_view_util.py) catches what it is for: torch stand-ins for a kernel on CPU arenas — one correct, six wrong
in the ways a kernel on a strided view goes wrong — in all five storage types.  The stand-in "kernel" is a scale by two; it reaches memory the way a kernel does, through the arena's bytes at the view's pointer, pitch and offsets."""
import pytest
import torch

from tests import _view_util as V

N, C, H, W = 2, 16, 3, 5
IDS = ["f32", "bf16", "f16", "f16x2", "fp8"]


def _arenas(dtype):
    es = V.ESIZE[dtype]
    g = torch.Generator().manual_seed(7)
    x = torch.randint(-8, 9, (N, C, H, W), generator=g).float() / 4  # exact in every storage type, doubled too
    xin = V.carve((N, C, H, W), dtype, "cpu", 16, C * es + 32, "in")
    V.write(xin, x)
    xin.arena.seal()
    y = V.carve((N, C, H, W), dtype, "cpu", 32, C * es + 64, "out")
    return x, xin.arena, y.arena


def _store(a, pixel, channel, src):
    for dst, s in zip(V.elem_bytes(a, pixel, channel), src):
        dst.copy_(s)


def kernel(xa, ya, fault=None):
    x = V.decode(xa.own, xa.shape, xa.dtype)
    y = 2.0 * x
    rows = y.permute(0, 2, 3, 1).reshape(-1, C)  # (a view of y)
    if fault == "reads_neighbour_channel":  # channel C of pixel 3 (the neighbour's first) times a zero weight, into channel C - 1
        rows[3, C - 1] += V.load_elem(xa, 3, C) * 0.0
    if fault == "reads_pixel_in_front":  # pixel -1 (in front of image 0), channel 2, times zero, into pixel 0
        rows[0, 2] += V.load_elem(xa, -1, 2) * 0.0
    ya.own.copy_(V.encode(rows.view(N, H, W, C).permute(0, 3, 1, 2), ya.dtype))
    if fault == "unwritten":
        _store(ya, 7, 11, [torch.full_like(p, V.NAN_BYTE) for p in V.elem_bytes(ya, 7, 11)])
    if fault == "stores_neighbour_channel":
        _store(ya, 4, C, V.elem_bytes(ya, 4, 0))
    if fault == "stores_guard_pixel":
        _store(ya, N * H * W + 1, 5, V.elem_bytes(ya, 0, 5))
    if fault == "stores_zero_padding":
        ya.raw2d[ya.guard + 9, ya.ld_b - 16:].zero_()  # the last 16 bytes of pixel 9's pitch
    if fault == "writes_source":
        _store(xa, 2, 1, V.elem_bytes(xa, 2, 0))


def _audit(x, xa, ya):
    """What every containment test asserts, as (check, location) of the first failure or None."""
    for name, loc in (("nan", V.first_nan(V.read(ya))), ("out_touched", V.first_touched(ya)), ("in_touched", V.first_touched(xa))):
        if loc is not None:
            return name, loc
    assert torch.equal(V.read(ya), 2.0 * x)
    return None


@pytest.mark.parametrize("dtype", V.STORAGE_TYPES, ids=IDS)
def test_correct_stand_in_passes(dtype):
    x, xa, ya = _arenas(dtype)
    kernel(xa, ya)
    assert _audit(x, xa, ya) is None
    V.check_untouched(xa)
    V.check_untouched(ya)
    V.check_no_nan(ya)


def _pad_channel(dtype):
    """Channel index (relative to the view) of the first of the pitch's last 16 bytes: the view sits at 32 bytes, 32 more follow it."""
    return C if dtype == V.F16X2 else C + 16 // V.ESIZE[dtype]  # (split float16: those bytes are the lo chunk of the group behind the view)


WRONG = [
    ("stores_neighbour_channel", "out_touched", lambda dt: (4, C)),
    ("stores_guard_pixel", "out_touched", lambda dt: (N * H * W + 1, 5)),
    ("stores_zero_padding", "out_touched", lambda dt: (9, _pad_channel(dt))),
    ("unwritten", "nan", lambda dt: (7, 11)),
    ("reads_neighbour_channel", "nan", lambda dt: (3, C - 1)),
    ("reads_pixel_in_front", "nan", lambda dt: (0, 2)),
    ("writes_source", "in_touched", lambda dt: (2, 1)),
]


@pytest.mark.parametrize("dtype", V.STORAGE_TYPES, ids=IDS)
@pytest.mark.parametrize("fault,check,where", WRONG, ids=[f[0] for f in WRONG])
def test_wrong_stand_in_is_reported_where_it_went_wrong(fault, check, where, dtype):
    x, xa, ya = _arenas(dtype)
    kernel(xa, ya, fault)
    assert _audit(x, xa, ya) == (check, where(dtype))
    with pytest.raises(AssertionError):
        V.check_untouched(xa)
        V.check_untouched(ya)
        V.check_no_nan(ya)


@pytest.mark.parametrize("dtype", V.STORAGE_TYPES, ids=IDS)
def test_arena_fill_is_nan_everywhere_around_an_input_and_guards_are_wide_enough(dtype):
    x, xa, ya = _arenas(dtype)
    assert xa.guard >= W + 2 and ya.guard >= W + 2
    es = V.ESIZE[dtype]
    ring = xa.raw.clone()
    ring.view(-1, xa.ld_b)[xa.guard: xa.guard + xa.npix, xa.c_off_b: xa.c_off_b + C * es] = V.NAN_BYTE
    if dtype == V.F16X2:
        assert bool(torch.isnan(ring.view(torch.float16).float()).all())  # both halves
    else:
        assert bool(torch.isnan(ring.view(dtype).float()).all())
    assert xa.view.data_ptr() % 16 == 0 and ya.view.data_ptr() % 16 == 0
    assert xa.view.data_ptr() - xa.raw.data_ptr() == xa.guard * xa.ld_b + 16
    assert tuple(xa.view.shape) == (N, C, H, W) and xa.view.stride(1) == 1 and xa.view.stride(3) * es == xa.ld_b
    assert torch.equal(V.read(xa), x) and torch.equal(V.rounded(x, dtype), x)
