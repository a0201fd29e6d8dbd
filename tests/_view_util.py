"""Containment harness for kernels that run on strided NHWC views (not collected; works on any device).

An *arena* is ONE allocation of bytes that holds a view with guards around it: ``guard`` pixels of the view's pitch in front of its first
pixel and behind its last, the channels in front of ``c_off`` and the rest of the pitch behind the view's own ``c`` channels.  Everything
a kernel may read by mistake is a NaN, everything it may store by mistake lands in bytes the test owns and compares afterwards:

  role "in"   every byte outside the view's own elements is 0xFF (a NaN in fp32, bf16, fp16, both halves of split float16 and e4m3fn);
              the caller fills the view with its data (``write``) and calls ``seal``: after the launch the WHOLE arena must be unchanged.
  role "out"  every byte outside the view is 0xA5, the view's own elements are 0xFF: an element nobody stored reads back as NaN.

Locations are reported as (pixel, channel) relative to the view: pixel 0 is its first pixel (guard pixels in front are negative, those
behind start at n * h * w), channel 0 its first channel (negative: the channels in front of the slice, >= c: the neighbour / pitch padding).
No view is placed at an end of its allocation: nothing here can make a load or store fault.
"""
import torch

FP8 = torch.float8_e4m3fn
F16X2 = torch.complex32  # split float16 (a container: per 8 channels [hi x 8 | lo x 8] halves, x ~= hi + lo * 2^-11)
ESIZE = {torch.float32: 4, torch.bfloat16: 2, torch.float16: 2, FP8: 1, F16X2: 4}
STORAGE_TYPES = [torch.float32, torch.bfloat16, torch.float16, F16X2, FP8]
NAN_BYTE, OUT_GUARD_BYTE = 0xFF, 0xA5
# For kernels that take a maximum (a max ignores NaN): 0x7B bytes are a large positive number in every 16- and 32-bit type — 61,280 in fp16,
# 1.3e36 in bf16 and fp32 — so a guard that is read wins the maximum and shows in the result.
BIG_BYTE = 0x7B


class Arena:
    def __init__(self, raw, view, shape, dtype, c_off_b, ld_b, guard, role, fill=None):
        self.raw, self.view, self.shape, self.dtype, self.role = raw, view, tuple(shape), dtype, role
        self.c_off_b, self.ld_b, self.guard, self.es = c_off_b, ld_b, guard, ESIZE[dtype]
        n, c, h, w = shape
        self.npix, self.c = n * h * w, c
        self.fill = fill if fill is not None else NAN_BYTE if role == "in" else OUT_GUARD_BYTE
        self.sealed = None

    @property
    def raw2d(self):
        """The arena as (pixels, pitch bytes), guard pixels included."""
        return self.raw.view(-1, self.ld_b)

    @property
    def own(self):
        """The view's own elements as a strided (n * h * w, c * element size) uint8 view of the arena."""
        return self.raw2d[self.guard: self.guard + self.npix, self.c_off_b: self.c_off_b + self.c * self.es]

    def seal(self):
        """Remember the arena as it is now: ``check_untouched`` then also holds the view's own elements to it (a source nobody may write)."""
        self.sealed = self.raw.clone()
        return self

    def _where(self, flat_byte):
        p, b = divmod(int(flat_byte), self.ld_b)
        b -= self.c_off_b
        if self.dtype == F16X2:  # 32 bytes per 8 channels: a chunk of hi halves, then a chunk of lo halves
            return p - self.guard, (b // 32) * 8 + (b % 16) // 2
        return p - self.guard, b // self.es


def carve(shape_nchw, dtype, device, c_off, ld, role, guard=None, aligned=True, fill=None):
    """An NHWC view (n, c, h, w) of ``dtype`` at channel offset ``c_off`` BYTES with pixel pitch ``ld`` BYTES inside a fresh arena; the arena
    is ``view.arena``.  ``aligned``: hold c_off and ld to the 16 bytes the library's vector paths need (False: the scalar-store output form).
    ``fill``: another byte than the role's for everything outside the view's elements (``BIG_BYTE`` for the sources of max pools)."""
    n, c, h, w = shape_nchw
    es = ESIZE[dtype]
    assert role in ("in", "out") and c_off % es == 0 and ld % es == 0 and c_off + c * es <= ld
    assert not aligned or (c_off % 16 == 0 and ld % 16 == 0), "c_off and ld are multiples of 16 bytes"
    guard = 2 * (w + 2) if guard is None else guard
    assert guard >= w + 2
    npix = n * h * w
    raw = torch.full(((2 * guard + npix) * ld,), fill if fill is not None else NAN_BYTE if role == "in" else OUT_GUARD_BYTE, dtype=torch.uint8, device=device)
    flat = raw[guard * ld + c_off:].view(dtype)
    lde = ld // es
    view = flat.as_strided((n, c, h, w), (h * w * lde, 1, w * lde, lde))
    a = Arena(raw, view, shape_nchw, dtype, c_off, ld, guard, role, fill)
    if role == "out":
        a.own.fill_(NAN_BYTE)
    view.arena = a
    return view


def _arena(v):
    return v if isinstance(v, Arena) else v.arena


def elem_bytes(v, pixel, channel):
    """The byte ranges (one; split float16: the hi and the lo half) of element (pixel, channel) RELATIVE to the view — any pixel and channel
    the arena holds, guards and neighbours included, the way a kernel's pointer arithmetic reaches them."""
    a = _arena(v)
    o = (a.guard + pixel) * a.ld_b + a.c_off_b
    if a.dtype == F16X2:
        o += (channel // 8) * 32 + (channel % 8) * 2
        return [a.raw[o: o + 2], a.raw[o + 16: o + 18]]
    o += channel * a.es
    return [a.raw[o: o + a.es]]


def load_elem(v, pixel, channel):
    """The value a kernel gets when it loads element (pixel, channel) relative to the view (see ``elem_bytes``)."""
    a = _arena(v)
    parts = [p.clone() for p in elem_bytes(a, pixel, channel)]
    if a.dtype == F16X2:
        hi, lo = (float(p.view(torch.float16)) for p in parts)
        return hi + lo / 2048.0
    return float(parts[0].view(a.dtype).float())


def first_touched(v):
    """(pixel, channel) of the first byte outside the view's own elements that differs from the arena's fill — for a sealed arena: of the
    first byte anywhere that differs from the sealed copy — or None."""
    a = _arena(v)
    if a.sealed is not None:
        bad = a.raw != a.sealed
    else:
        bad = (a.raw != a.fill).view(-1, a.ld_b).clone()
        bad[a.guard: a.guard + a.npix, a.c_off_b: a.c_off_b + a.c * a.es] = False
        bad = bad.view(-1)
    if not bool(bad.any()):
        return None
    return a._where(torch.nonzero(bad)[0, 0])


def check_untouched(v, what="arena"):
    loc = first_touched(v)
    a = _arena(v)
    assert loc is None, (f"{what}: a byte {'of a source' if a.sealed is not None else 'outside the view'} was written, first at pixel {loc[0]} "
                         f"(view has {a.npix}), channel {loc[1]} (view has {a.c})")


def first_nan(t):
    """(pixel, channel) of the first NaN of a real (n, c, h, w) tensor, or None."""
    n, c, h, w = t.shape
    bad = torch.isnan(t.float()).permute(0, 2, 3, 1).reshape(n * h * w, c)
    if not bool(bad.any()):
        return None
    p, ch = torch.nonzero(bad)[0].tolist()
    return p, ch


def check_no_nan(v, got=None, what="output"):
    """No element of an "out" view reads back as NaN: none was left unstored (the 0xFF fill) and none was computed from a guard byte."""
    loc = first_nan(read(v) if got is None else got)
    assert loc is None, f"{what}: NaN at pixel {loc[0]}, channel {loc[1]} (an element was never stored, or a guard byte was consumed)"


# ---- values in and out of a view, through the arena's bytes (no arithmetic on the container types) ---------------------------------


def encode(t, dtype):
    """Real (n, c, h, w) values -> (n * h * w, c * element size) uint8 rows in the storage type's NHWC memory layout."""
    n, c, h, w = t.shape
    rows = t.permute(0, 2, 3, 1).reshape(n * h * w, c)
    if dtype == F16X2:
        assert c % 8 == 0
        x = rows.float()
        hi = x.half()
        lo = ((x - hi.float()) * 2048.0).half()
        rows = torch.stack((hi.view(-1, c // 8, 8), lo.view(-1, c // 8, 8)), dim=2).reshape(n * h * w, 2 * c)
    else:
        rows = rows.to(dtype)
    return rows.contiguous().view(torch.uint8).view(n * h * w, -1)


def decode(rows, shape, dtype):
    """The inverse of ``encode``: uint8 rows -> fp32 (n, c, h, w) (split float16: hi + lo * 2^-11 in fp64, rounded to fp32)."""
    n, c, h, w = shape
    rows = rows.contiguous()
    if dtype == F16X2:
        hv = rows.view(torch.float16).view(n * h * w, c // 8, 2, 8).double()
        val = (hv[:, :, 0] + hv[:, :, 1] / 2048.0).reshape(n * h * w, c).float()
    else:
        val = rows.view(dtype).view(n * h * w, c).float()
    return val.view(n, h, w, c).permute(0, 3, 1, 2)


def write(v, t):
    """Store real (n, c, h, w) values into the view (rounded to its storage type); returns the view."""
    a = _arena(v)
    assert tuple(t.shape) == a.shape
    a.own.copy_(encode(t.to(a.raw.device), a.dtype))
    return a.view


def read(v):
    a = _arena(v)
    return decode(a.own, a.shape, a.dtype)


def rounded(t, dtype):
    """What a view of ``dtype`` holds after ``write(view, t)``, as fp32 on t's device."""
    return decode(encode(t, dtype), t.shape, dtype)


# ---- the views the containment tests use ----------------------------------------------------------------------------------------------------


def _up16(nbytes):
    return -(-nbytes // 16) * 16


def source(t, dtype, device, c_off=16, extra=32, fill=None):
    """Real (n, c, h, w) values -> a sealed "in" view on ``device``: a slice at ``c_off`` bytes of a pitch ``extra`` bytes wider than its channels."""
    n, c, h, w = t.shape
    v = carve((n, c, h, w), dtype, device, c_off, _up16(c * ESIZE[dtype]) + extra, "in", fill=fill)
    write(v, t)
    v.arena.seal()
    return v


def dest(shape, dtype, device, c_off=32, extra=64):
    """An "out" view: a slice at ``c_off`` bytes of a pitch ``extra`` bytes wider than its channels."""
    return carve(shape, dtype, device, c_off, _up16(shape[1] * ESIZE[dtype]) + extra, "out")


def inout(t, dtype, device, c_off=32, extra=64):
    """An "out" view that already holds ``t`` (an operand a launch adds into): its surroundings are checked, its elements are the result."""
    v = dest(tuple(t.shape), dtype, device, c_off, extra)
    write(v, t)
    return v
