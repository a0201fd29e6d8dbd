"""The entry points beside ``dy_conv2d_nhwc`` that take a pixel pitch, on views carved out of arenas (tests/_view_util.py): every source a channel
slice at 16 bytes of a pitch 32 bytes wider than its channels with NaN bytes all round it, every destination a slice at 32 bytes of a pitch
64 bytes wider, 0xA5 around it and NaN inside.  Per launch: the result against the reference of the entry point's own parity test, to that
test's tolerance; no NaN in it; no byte of a destination arena outside the view changed; no byte of a source arena changed.

Shapes: the channel counts of the smallest case of each parity test, on maps with odd H and W and a batch of at least 2 (partial tiles in both
directions and an image boundary).  Where the Python wrapper of an entry point allocates its result itself, ``arena_results`` makes that allocation
an arena view too, so every launch here stores into memory the test owns; the contiguous ``pred`` tensors of the Detect launches lie between guards."""
import contextlib
import math

import pytest
import torch
import torch.nn.functional as F

from drone_yolo_amd import hip_ops as H
from oracle import drone_yolo_oracle as O
from tests import _view_util as V
from tests._util import quantize
from tests.test_kernels_gpu import check_close
from tests.test_train_gpu import close

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]
BITS16 = [torch.bfloat16, torch.float16]
# One rounding to nearest of the storage type is at most half an ulp, 2^-9 (bf16) / 2^-11 (fp16) of the value; twice that is allowed.  fp32: a sum
# of four fp32 values in another order, 4 ulps of the largest.
ONE_ROUNDING = {torch.float32: 2.0 ** -21, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10}


def sync_and_check(outs=(), ins=()):
    """(b), (c), (d) for one or several launches; returns the destinations' values on the CPU."""
    torch.cuda.synchronize()
    for i, v in enumerate(outs):
        V.check_untouched(v, f"destination arena {i}")
    for i, v in enumerate(ins):
        V.check_untouched(v, f"source arena {i}")
    got = [V.read(v).cpu() for v in outs]
    for i, (v, t) in enumerate(zip(outs, got)):
        V.check_no_nan(v, t, f"destination {i}")
    return got


def no_nan(t, what):
    loc = V.first_nan(t) if t.dim() == 4 else (None if not bool(torch.isnan(t.float()).any()) else tuple(torch.nonzero(torch.isnan(t.float()))[0].tolist()))
    assert loc is None, f"{what}: NaN at {loc} (a guard byte was consumed)"


@contextlib.contextmanager
def arena_results(monkeypatch):
    """Inside, every ``hip_ops.alloc_nhwc`` (the results that upsample2x_bwd, head_grad_split, conv_grouped_bwd and stem_conv_u8 allocate themselves)
    is a ``V.dest`` view: the kernel gets that view's pointer and pitch.  Yields the list of the views made."""
    made = []

    def alloc(n, c, h, w, dtype, device, ld=None):
        made.append(V.dest((n, c, h, w), dtype, device))
        return made[-1]

    with monkeypatch.context() as m:
        m.setattr(H, "alloc_nhwc", alloc)
        yield made


def between_guards(shape, dtype, device):
    """A CONTIGUOUS tensor (a ``pred`` of the Detect launches) in the middle of one allocation: 0xA5 in front of and behind it, NaN inside;
    returns (tensor, whole buffer, copy of the buffer with the tensor's bytes zeroed for the comparison afterwards)."""
    nbytes = math.prod(shape) * V.ESIZE[dtype]
    pad = 4096
    raw = torch.full((2 * pad + nbytes,), V.OUT_GUARD_BYTE, dtype=torch.uint8, device=device)
    raw[pad: pad + nbytes] = V.NAN_BYTE
    return raw[pad: pad + nbytes].view(dtype).view(shape), raw, pad


def guards_untouched(raw, pad, what):
    assert bool((raw[:pad] == V.OUT_GUARD_BYTE).all()) and bool((raw[-pad:] == V.OUT_GUARD_BYTE).all()), f"{what}: a byte in front of or behind the tensor was written"


def test_the_harness_sees_a_real_launch_that_leaves_its_view(device):
    """Positive control on the device: dy_copy_nhwc asked for 24 channels of 16-channel views (the 8 behind them still inside both arenas' pitches)
    loads the source's NaN neighbours and stores them behind the destination: reported at pixel 0, channel 16 — and a launch kept to 16 channels is not."""
    t = quantize(torch.randn(2, 16, 5, 7, generator=torch.Generator().manual_seed(1)), torch.bfloat16)
    x, y = V.source(t, torch.bfloat16, device), V.dest((2, 16, 5, 7), torch.bfloat16, device)
    H.copy_nhwc(x, y)
    got, = sync_and_check([y], [x])
    assert torch.equal(got, t)
    H.copy_nhwc(x.as_strided((2, 24, 5, 7), x.stride()), y.as_strided((2, 24, 5, 7), y.stride()))
    torch.cuda.synchronize()
    assert V.first_touched(y) == (0, 16) and V.first_touched(x) is None
    with pytest.raises(AssertionError, match="pixel 0 .*channel 16"):
        V.check_untouched(y)
    stray = V.decode(y.arena.raw2d[y.arena.guard: y.arena.guard + 70, 32 + 32: 32 + 48], (2, 8, 5, 7), torch.bfloat16)
    assert bool(torch.isnan(stray).all())  # what it stored there are the source's guard bytes


# ---- inference copies and pools ------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_upsample_copy_and_pools_on_views(dtype, device):
    g = torch.Generator().manual_seed(13)
    t = quantize(torch.randn(2, 16, 7, 5, generator=g), dtype)
    x = V.source(t, dtype, device)
    up, cp = V.dest((2, 16, 14, 10), dtype, device), V.dest((2, 16, 7, 5), dtype, device)
    H.upsample2x(x, out=up)
    H.copy_nhwc(x, cp)
    got_up, got_cp = sync_and_check([up, cp], [x])
    assert torch.equal(got_up, F.interpolate(t, scale_factor=2.0, mode="nearest")) and torch.equal(got_cp, t)
    # SPPF: the three pools write slices of the buffer the source is a slice of (one pitch): four slices of one arena.  A max ignores NaN, so
    # this arena is filled with 0x7B bytes all round and inside: 61,280 in fp16, 1.3e36 in bf16 and fp32 — a pool that reads a pixel or channel
    # outside its source has it as its maximum
    s = quantize(torch.randn(2, 16, 7, 9, generator=g), dtype)
    buf = V.carve((2, 64, 7, 9), dtype, device, 32, 64 * V.ESIZE[dtype] + 64, "in", fill=V.BIG_BYTE)
    parts = [buf[:, 16 * i: 16 * (i + 1)] for i in range(4)]
    buf.arena.own.view(-1, 4, 16 * V.ESIZE[dtype])[:, 0].copy_(V.encode(s, dtype).to(device))
    H.sppf_maxpool3(*parts, 5)
    got, = sync_and_check([buf])
    assert torch.equal(got[:, :16], s), "the pools wrote their source"
    assert float(got.abs().max()) < 100.0, "a pool consumed a guard value or left an element unstored"
    p = s
    for i in range(3):
        p = F.max_pool2d(p, 5, 1, 2)
        assert torch.equal(got[:, 16 * (i + 1): 16 * (i + 2)], p), f"sppf pass {i}"


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_quantize_fp8_and_depth_to_space_on_views(dtype, device):
    g = torch.Generator().manual_seed(3)
    t = quantize(torch.randn(2, 32, 9, 11, generator=g) * 30, dtype)
    t[0, 0, 0, 0], t[0, 1, 0, 0] = 1e4, -1e4  # saturate
    x = V.source(t, dtype, device)
    q = V.dest((2, 32, 9, 11), H.FP8, device)
    H.set_fp8_act_scale(0.25)
    try:
        H.quantize_fp8(x, out=q)
        got, = sync_and_check([q], [x])
    finally:
        H.set_fp8_act_scale(1.0)
    assert torch.equal(got, (t / 0.25).clamp(-448, 448).to(H.FP8).float())
    n, c, h, w = 3, 24, 5, 7
    t = quantize(torch.randn(n, 4 * c, h, w, generator=g), dtype)
    x, y = V.source(t, dtype, device), V.dest((n, c, 2 * h, 2 * w), dtype, device)
    H.depth_to_space2(x, out=y)
    got, = sync_and_check([y], [x])
    assert torch.equal(got, t.reshape(n, 2, 2, c, h, w).permute(0, 3, 4, 1, 5, 2).reshape(n, c, 2 * h, 2 * w))


# ---- inference launches ----------------------------------------------------------------------------------------------------------------------


def _image_between_guards(img, fill, device):
    """A contiguous NCHW image in the middle of one allocation, ``fill`` bytes in front of and behind it (the stems take no pitch: the image is
    read as it lies); returns (image view, whole buffer)."""
    nbytes = img.numel() * img.element_size()
    pad = 4096
    raw = torch.full((2 * pad + nbytes,), fill, dtype=torch.uint8, device=device)
    view = raw[pad: pad + nbytes].view(img.dtype).view(img.shape)
    view.copy_(img)
    return view, raw


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_stem_conv_on_views(dtype, device):
    n, cin, h, w, cout = 2, 3, 33, 31, 16
    g = torch.Generator().manual_seed(h * 7 + cout)
    img = torch.rand(n, cin, h, w, generator=g)
    wt = quantize(torch.randn(cout, cin, 3, 3, generator=g) * 0.4, dtype)
    bias = torch.randn(cout, generator=g) * 0.2
    src, raw = _image_between_guards(img, V.NAN_BYTE, device)
    before = raw.clone()
    y = V.dest((n, cout, 17, 16), dtype, device)
    H.stem_conv(src, H.PackedStem(wt, bias, True, dtype, device), out=y)
    got, = sync_and_check([y])
    assert torch.equal(raw, before), "the stem wrote its image"
    check_close(got, F.silu(F.conv2d(quantize(img, dtype), wt, bias, 2, 1)), dtype, "stem on a view")


@pytest.mark.parametrize("dtype", BITS16, ids=["bf16", "f16"])
def test_stem_conv_u8_on_views(dtype, device, monkeypatch):
    n, h, w = 2, 33, 37
    g = torch.Generator().manual_seed(h)
    img = torch.randint(0, 256, (n, 3, h, w), generator=g, dtype=torch.uint8)
    wt = (torch.randn(32, 3, 3, 3, generator=g) * 0.2).to(device)
    src, raw = _image_between_guards(img, V.NAN_BYTE, device)  # (255 around the image: a pixel read from there is 1.0 where the padding's 0 belongs)
    before = raw.clone()
    with arena_results(monkeypatch) as made:
        z = H.stem_conv_u8(src, wt, dtype)
    assert len(made) == 1 and z is made[0]
    got, = sync_and_check([z])
    assert torch.equal(raw, before), "the stem wrote its image"
    close(got, F.conv2d(quantize(img.float() / 255.0, dtype), quantize(wt.cpu(), dtype), None, 2, 1), dtype, "stem u8")


def _c2f_weights(cin, g, dtype):
    q = lambda t: quantize(t, dtype)  # noqa: E731
    mk = lambda co, ci, k: (q(torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5), torch.randn(co, generator=g) * 0.2)  # noqa: E731
    return mk(64, cin, 1), mk(32, 32, 3), mk(32, 32, 3), mk(64, 96, 1)


def _c2f_reference(x, ws, shortcut, dtype):
    """The CPU chain of test_c2f_fused_block_matches_cpu_chain_and_layerwise: every intermediate rounded to the storage type."""
    q = lambda t: quantize(t, dtype)  # noqa: E731
    (w1, b1), (wa, ba), (wb, bb), (w2, b2) = ws
    y = q(F.silu(F.conv2d(x, w1, b1)))
    y0, y1 = y[:, :32], y[:, 32:]
    t = q(F.silu(F.conv2d(y1, wa, ba, 1, 1)))
    y2 = F.silu(F.conv2d(t, wb, bb, 1, 1))
    y2 = q(y2 + y1) if shortcut else q(y2)
    return q(F.silu(F.conv2d(torch.cat((y0, y1, y2), 1), w2, b2)))


@pytest.mark.parametrize("dtype", BITS16, ids=["bf16", "f16"])
@pytest.mark.parametrize("with_lo", [False, True], ids=["plain", "x_lo"])
def test_c2f_fused_on_views(with_lo, dtype, device):
    g = torch.Generator().manual_seed(41 + with_lo)
    n = 2
    if with_lo:  # (the block's map is twice the odd half-resolution one)
        x_lo, x_hi = quantize(torch.randn(n, 128, 9, 7, generator=g), dtype), quantize(torch.randn(n, 64, 18, 14, generator=g), dtype)
        x = torch.cat((F.interpolate(x_lo, scale_factor=2, mode="nearest"), x_hi), 1)
        assert H.c2f_fused_supported(192, 32, 64, 1, dtype, cin_lo=128)
    else:
        x = x_hi = quantize(torch.randn(n, 64, 15, 17, generator=g), dtype)
        assert H.c2f_fused_supported(64, 32, 64, 1, dtype)
    ws = _c2f_weights(x.shape[1], g, dtype)
    pk = H.PackedC2f(*ws, shortcut=True, dtype=dtype, device=device)
    ins = [V.source(x_hi, dtype, device)] + ([V.source(x_lo, dtype, device)] if with_lo else [])
    y = V.dest((n, 64) + tuple(x.shape[2:]), dtype, device)
    H.c2f_fused(ins[0], pk, out=y, x_lo=ins[1] if with_lo else None)
    got, = sync_and_check([y], ins)
    check_close(got, _c2f_reference(x, ws, True, dtype), dtype, "fused C2f on views", extra=3.0)


@pytest.mark.parametrize("dtype", BITS16, ids=["bf16", "f16"])
def test_detect_branch_fused_on_views(dtype, device):
    """Both kinds (1: box, 2: class) of dy_detect_branch_fused on one level, against the CPU chain of test_detect_branch_fused_matches_cpu_chain from
    the branches' first-conv outputs on: 3x3 + SiLU rounded to the storage type, the plain 1x1 in float64, the oracle's decode."""
    g = torch.Generator().manual_seed(17)
    n, h, w, nc, stride = 3, 5, 3, 10, 8.0
    q = lambda t: quantize(t, dtype)  # noqa: E731
    xs = [q(torch.randn(n, 64, h, w, generator=g)) for _ in range(2)]
    w3 = [q(torch.randn(64, 64, 3, 3, generator=g) * 0.06) for _ in range(2)]
    b3 = [torch.randn(64, generator=g) * 0.2 for _ in range(2)]
    w1 = [q(torch.randn(co, 64, 1, 1, generator=g) * 0.2) for co in (64, nc)]
    b1 = [torch.randn(64, generator=g), torch.randn(nc, generator=g) - 1.0]
    assert all(H.branch_fused_supported(64, 64, co, kind, nc, 16, dtype) for co, kind in ((64, 1), (nc, 2)))
    feats = [F.conv2d(q(F.silu(F.conv2d(xs[i], w3[i], b3[i], 1, 1))).double(), w1[i].double(), b1[i].double()).float() for i in range(2)]
    ref = O.detect_decode([torch.cat(feats, 1)], [stride], nc)
    # the level's 15 anchors in the middle of a wider pred (37 in front, 12 behind, as another level's would be), pred itself between guards
    a0, A = 37, 37 + h * w + 12
    pred, raw, pad = between_guards((n, 4 + nc, A), torch.float32, device)
    pred[:, :, :a0] = -7.0
    pred[:, :, a0 + h * w:] = -7.0
    ins = [V.source(t, dtype, device) for t in xs]
    for i, kind in enumerate((1, 2)):
        pc3 = H.PackedConv(w3[i], b3[i], 1, 1, 1, True, dtype, device, halo=True)
        wp, bp = H.pack_frag1x1(w1[i], b1[i], dtype, device)
        H.detect_branch_fused(ins[i], pc3, wp, bp, kind, nc, 16, stride, pred, a0)
    sync_and_check([], ins)
    guards_untouched(raw, pad, "pred")
    assert bool((pred[:, :, :a0] == -7.0).all()) and bool((pred[:, :, a0 + h * w:] == -7.0).all()), "a row was written outside the level's anchors"
    y = pred[:, :, a0: a0 + h * w].cpu()
    no_nan(y, "decoded rows")
    box_tol = (0.03 if dtype == torch.bfloat16 else 0.004) * float(ref[:, :4].abs().max())
    cls_tol = 0.03 if dtype == torch.bfloat16 else 0.004
    assert float((y[:, :4] - ref[:, :4]).abs().max()) <= box_tol and float((y[:, 4:] - ref[:, 4:]).abs().max()) <= cls_tol


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_detect_head_decode_on_views(dtype, device):
    g = torch.Generator().manual_seed(41)
    nc, c_cls, n = 10, 64, 3
    shapes, strides = [(5, 7), (3, 3), (1, 1)], [4.0, 8.0, 16.0]
    rnd = lambda t: t.to(dtype).float()  # noqa: E731
    xb = [rnd(torch.randn(n, 64, h, w, generator=g)) for h, w in shapes]
    xc = [rnd(torch.randn(n, c_cls, h, w, generator=g)) for h, w in shapes]
    wb = [rnd(torch.randn(64, 64, 1, 1, generator=g) * 0.25) for _ in shapes]
    wc = [rnd(torch.randn(nc, c_cls, 1, 1, generator=g) * 0.2) for _ in shapes]
    bb = [torch.randn(64, generator=g) for _ in shapes]
    bc = [torch.randn(nc, generator=g) - 1.0 for _ in shapes]
    feats = [torch.cat([F.conv2d(xb[i].double(), wb[i].double(), bb[i].double()), F.conv2d(xc[i].double(), wc[i].double(), bc[i].double())], 1).float()
             for i in range(len(shapes))]
    ref = O.detect_decode(feats, strides, nc)
    assert H.head_decode_supported(64, c_cls, nc, 16, dtype)
    dxb, dxc = [V.source(t, dtype, device) for t in xb], [V.source(t, dtype, device) for t in xc]
    pb = [H.pack_frag1x1(wb[i], bb[i], dtype, device) for i in range(len(shapes))]
    pc = [H.pack_frag1x1(wc[i], bc[i], dtype, device) for i in range(len(shapes))]
    out, raw, pad = between_guards((n, 4 + nc, sum(h * w for h, w in shapes)), torch.float32, device)
    y = H.detect_head_decode(dxb, dxc, pb, pc, strides, nc, 16, out=out)
    sync_and_check([], dxb + dxc)
    guards_untouched(raw, pad, "decoded rows")
    no_nan(y.cpu(), "decoded rows")
    assert torch.allclose(y.cpu(), ref, rtol=1e-4, atol=2e-3), float((y.cpu() - ref).abs().max())


# ---- training: BatchNorm and SiLU ------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bn_train_forward_backward_on_views(dtype, device):
    g = torch.Generator().manual_seed(96)
    shape = n, c, h, w = 2, 96, 17, 13
    z = quantize(torch.randn(shape, generator=g) * 1.7 + torch.randn(1, c, 1, 1, generator=g), dtype).requires_grad_(True)
    gamma, beta = (torch.rand(c, generator=g) + 0.5).requires_grad_(True), (torch.randn(c, generator=g) * 0.3).requires_grad_(True)
    y = F.silu(F.batch_norm(z, None, None, gamma, beta, training=True, momentum=0.03, eps=1e-3))
    dy = quantize(torch.randn(shape, generator=g), dtype)
    y.backward(dy)
    st = H.BnState(c, device)
    zd, dyd = V.source(z.detach(), dtype, device), V.source(dy, dtype, device)
    yd, dzd = V.dest(shape, dtype, device), V.dest(shape, dtype, device)
    gd, bd = gamma.detach().to(device), beta.detach().to(device)
    H.bn_train_fwd(zd, gd, bd, st, True, out=yd)
    _, dgam, dbet = H.bn_train_bwd(dyd, zd, gd, bd, st, True, out=dzd)
    got_y, got_dz = sync_and_check([yd, dzd], [zd, dyd])
    close(got_y, y.detach(), dtype, "bn fwd")
    assert torch.allclose(st.mean.cpu(), z.detach().mean((0, 2, 3)), atol=1e-4, rtol=1e-4)
    close(got_dz, z.grad, dtype, "bn dz", extra=2.0)
    assert torch.allclose(dgam.cpu(), gamma.grad, rtol=2e-3, atol=2e-3 * float(gamma.grad.abs().max()))
    assert torch.allclose(dbet.cpu(), beta.grad, rtol=2e-3, atol=2e-3 * float(beta.grad.abs().max()))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bn_addend_and_silu_on_views(dtype, device):
    """silu(bn3(z3) + bn1(z1)) and its backward (test_two_branch_bn_sum_then_silu), each launch on arena views."""
    g = torch.Generator().manual_seed(5)
    shape = n, c, h, w = 3, 64, 19, 23
    z3 = quantize(torch.randn(shape, generator=g), dtype).requires_grad_(True)
    z1 = quantize(torch.randn(shape, generator=g) * 0.5, dtype).requires_grad_(True)
    g3, b3, g1, b1 = (torch.rand(c, generator=g) + 0.5 for _ in range(4))
    u = F.batch_norm(z3, None, None, g3, b3, True, 0.03, 1e-3) + F.batch_norm(z1, None, None, g1, b1, True, 0.03, 1e-3)
    y = F.silu(u)
    dy = quantize(torch.randn(shape, generator=g), dtype)
    y.backward(dy)
    s3, s1 = H.BnState(c, device), H.BnState(c, device)
    dev = lambda t: t.to(device)  # noqa: E731
    z3d, z1d, dyd = V.source(z3.detach(), dtype, device), V.source(z1.detach(), dtype, device), V.source(dy, dtype, device)
    u3 = H.bn_train_fwd(z3d, dev(g3), dev(b3), s3, False)
    torch.cuda.synchronize()
    u3d = V.source(u3.float().cpu(), dtype, device)  # the addend as a view of its own
    ud, yd, dud = V.dest(shape, dtype, device), V.dest(shape, dtype, device), V.dest(shape, dtype, device)
    H.bn_train_fwd(z1d, dev(g1), dev(b1), s1, False, addend=u3d, out=ud)
    sync_and_check([ud], [z1d, u3d])
    us = V.source(V.read(ud).cpu(), dtype, device)
    H.silu_fwd(us, out=yd)
    H.silu_bwd(us, dyd, out=dud)
    got_y, got_du = sync_and_check([yd, dud], [us, dyd])
    close(got_y, y.detach(), dtype, "repvgg fwd", extra=2.0)
    dus = V.source(got_du, dtype, device)
    dz3, dz1 = V.dest(shape, dtype, device), V.dest(shape, dtype, device)
    H.bn_train_bwd(dus, z3d, dev(g3), dev(b3), s3, False, out=dz3)
    H.bn_train_bwd(dus, z1d, dev(g1), dev(b1), s1, False, out=dz1)
    got3, got1 = sync_and_check([dz3, dz1], [dus, z3d, z1d])
    close(got3, z3.grad, dtype, "repvgg dz3", extra=3.0)
    close(got1, z1.grad, dtype, "repvgg dz1", extra=3.0)


# ---- training: gradients ---------------------------------------------------------------------------------------------------------------------


def _wgrad_atomics(xd, dzd, k, s, dtype, device):
    """dy_conv2d_wgrad_nhwc (no workspace: partial sums added with atomics) on the views, as test_wgrad_workspace_path_matches_atomics_and_autograd calls it."""
    import ctypes as C
    from drone_yolo_amd import _lib as L

    d = L.ConvDesc()
    (d.x, d.ld_x), (dzp, lddz) = H.view_params(xd), H.view_params(dzd)
    d.batch, d.cin, d.h, d.w_in = xd.shape
    d.cout, d.ho, d.wo = dzd.shape[1:]
    d.ksize, d.stride, d.pad, d.groups, d.dtype = k, s, k // 2, 1, H.dy_dtype(dtype)
    need = L.lib().dy_conv2d_wgrad_workspace_bytes(C.byref(d), lddz)
    dw = torch.zeros(d.cout, k, k, d.cin, device=device)
    assert L.lib().dy_conv2d_wgrad_nhwc(C.byref(d), dzp, lddz, dw.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    return dw.permute(0, 3, 1, 2), need


WGRAD = [(64, 16, 3, 1, 2, 15, 17, torch.bfloat16), (64, 16, 3, 1, 2, 15, 17, torch.float16), (64, 16, 3, 1, 2, 15, 17, torch.float32),
         (40, 24, 1, 1, 3, 33, 31, torch.bfloat16), (64, 128, 3, 2, 2, 21, 19, torch.bfloat16)]
# channel counts that are NOT whole 16-byte chunks: the launch reads the chunk's tail (include/dyolo.h: whatever it holds only reaches gradient entries
# that are never written) — here those tails are NaN
WGRAD_TAILS = [(20, 12, 3, 1, 2, 15, 17, torch.bfloat16), (20, 12, 1, 1, 2, 15, 17, torch.float16), (6, 10, 3, 1, 2, 15, 17, torch.float32), (12, 20, 3, 2, 2, 15, 17, torch.bfloat16),
               (3, 28, 3, 2, 2, 33, 37, torch.bfloat16)]  # (the last: the image stem's kernel, cin <= 8 and cout <= 32 at stride 2, on the image's own 3 channels)


@pytest.mark.parametrize("case", WGRAD + WGRAD_TAILS, ids=[f"{c[0]}->{c[1]} k{c[2]} s{c[3]} {str(c[7])[6:]}" + (" tails" if c in WGRAD_TAILS else "") for c in WGRAD + WGRAD_TAILS])
def test_conv_wgrad_on_views(case, device):
    cin, cout, k, s, b, h, w, dtype = case
    g = torch.Generator().manual_seed(cin + cout + h + k)
    x = quantize(torch.randn(b, cin, h, w, generator=g), dtype).requires_grad_(True)
    wt = quantize(torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5, dtype).requires_grad_(True)
    z = F.conv2d(x, wt, None, s, k // 2)
    dz = quantize(torch.randn(z.shape, generator=g), dtype)
    z.backward(dz)
    xd, dzd = V.source(x.detach(), dtype, device), V.source(dz, dtype, device)
    dw_ws = H.conv_wgrad(xd, dzd, k, s, k // 2)  # the workspace path where the call has one
    dw_at, need = _wgrad_atomics(xd, dzd, k, s, dtype, device)
    sync_and_check([], [xd, dzd])
    if (cin, cout, k) == (40, 24, 1):
        assert need > 0  # (the smallest case of the workspace test: both paths ran)
    extra = 30.0 if dtype == torch.float32 else 10.0
    for what, dw in (("workspace", dw_ws), ("atomics", dw_at)):
        no_nan(dw.cpu(), f"wgrad ({what})")
        close(dw, wt.grad, torch.float32, f"wgrad ({what}) {case}", extra=extra)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("cin,cout,k,s", [(64, 16, 3, 1), (32, 64, 3, 2), (192, 128, 1, 1)], ids=["3x3 s1", "3x3 s2", "1x1"])
def test_conv_dgrad_on_views(cin, cout, k, s, dtype, device):
    b, h, w = 2, 15, 17
    g = torch.Generator().manual_seed(cin + k + s)
    x = quantize(torch.randn(b, cin, h, w, generator=g), dtype).requires_grad_(True)
    wt = quantize(torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5, dtype).requires_grad_(True)
    z = F.conv2d(x, wt, None, s, k // 2)
    dz = quantize(torch.randn(z.shape, generator=g), dtype)
    z.backward(dz)
    prev = quantize(torch.randn(x.shape, generator=g), dtype)
    pc = H.pack_dgrad(wt.detach().to(device), s, dtype, device)
    shape = (b, cin, 2 * z.shape[2], 2 * z.shape[3]) if s == 2 else tuple(x.shape)  # (the zero-dilated gather gives an even map; the odd one is its crop)
    dzd, pv = V.source(dz, dtype, device), V.source(F.pad(prev, (0, shape[3] - w, 0, shape[2] - h)), dtype, device)
    dx, dx2 = V.dest(shape, dtype, device), V.dest(shape, dtype, device)
    H.conv_dgrad(dzd, pc, s, out=dx)
    H.conv_dgrad(dzd, pc, s, out=dx2, accumulate=pv)
    got, got2 = sync_and_check([dx, dx2], [dzd, pv])
    close(got[:, :, :h, :w], x.grad, dtype, "dgrad")
    close(got2[:, :, :h, :w], x.grad + prev, dtype, "dgrad + accumulate")


@pytest.mark.parametrize("dtype", BITS16, ids=["bf16", "f16"])
def test_conv_dgrad_bn_behind_on_views(dtype, device):
    """dy_conv_desc.bnb_z (test_input_gradient_epilogue_leaves_the_batchnorm_backward_sums): the gradient, the saved z and the result as arena views; the
    workspace behind the reported slots stays as it was."""
    c, c2, b, h, w, act = 64, 64, 2, 17, 23, True
    g = torch.Generator().manual_seed(c + c2 + h)
    zc = quantize(torch.randn(b, c, h, w, generator=g) * 1.5 + 0.3, dtype)
    z = V.source(zc, dtype, device)
    gamma, beta = (torch.rand(c, generator=g) + 0.5).to(device), (torch.randn(c, generator=g) * 0.3).to(device)
    st = H.BnState(c, device)
    H.bn_train_fwd(z, gamma, beta, st, act)
    wt = quantize(torch.randn(c2, c, 3, 3, generator=g) * 0.06, dtype).to(device)
    dz2 = V.source(quantize(torch.randn(b, c2, h, w, generator=g), dtype), dtype, device)
    pc = H.pack_dgrad(wt.float(), 1, dtype, device)
    plain, dx = V.dest((b, c, h, w), dtype, device), V.dest((b, c, h, w), dtype, device)
    H.conv_dgrad(dz2, pc, 1, out=plain)
    torch.cuda.synchronize()
    st.ws.fill_(V.OUT_GUARD_BYTE)
    behind = H.BnBehind(z, gamma, beta, st, act)
    H.conv_dgrad(dz2, pc, 1, out=dx, bn_behind=behind)
    assert behind.slots > 0 and "bnb" in H.last_kernel_name(), (behind.slots, H.last_kernel_name())
    got_plain, got = sync_and_check([plain, dx], [dz2, z])
    assert torch.equal(got, got_plain)
    xg = torch.zeros(b, c, h, w, requires_grad=True)
    F.conv2d(xg, wt.cpu().float(), None, 1, 1).backward(V.read(dz2).cpu())
    close(got, xg.grad, dtype, "dgrad with the BatchNorm epilogue")
    assert bool((st.ws[(1 + behind.slots) * 2 * c * 8:] == V.OUT_GUARD_BYTE).all()), "the workspace behind the reported slots was written"
    part = st.ws.view(torch.float64)[2 * c: (1 + behind.slots) * 2 * c].view(behind.slots, 2 * c).sum(0).cpu()
    xh = (zc.double() - st.mean.double().cpu().view(1, -1, 1, 1)) * st.rstd.double().cpu().view(1, -1, 1, 1)
    u = gamma.double().cpu().view(1, -1, 1, 1) * xh + beta.double().cpu().view(1, -1, 1, 1)
    sg = torch.sigmoid(u)
    du = got.double() * (sg * (1 + u * (1 - sg)))
    ref = torch.cat([du.sum((0, 2, 3)), (du * xh).sum((0, 2, 3))])
    assert float((part - ref).abs().max()) <= 1e-4 * float(ref.abs().max()) + 1e-6, (part - ref).abs().max()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_grouped_bwd_head_split_colsum_on_views(dtype, device, monkeypatch):
    cin, cout, b, h, w = 16, 16, 2, 11, 13
    g_ = math.gcd(cin, cout)
    g = torch.Generator().manual_seed(cin + cout)
    x = quantize(torch.randn(b, cin, h, w, generator=g), dtype).requires_grad_(True)
    wt = (torch.randn(cout, cin // g_, 3, 3, generator=g) * 0.3).requires_grad_(True)
    z = F.conv2d(x, wt, None, 2, 1, groups=g_)
    dz = quantize(torch.randn(z.shape, generator=g), dtype)
    z.backward(dz)
    xd, dzd = V.source(x.detach(), dtype, device), V.source(dz, dtype, device)
    with arena_results(monkeypatch) as made:
        dw, dx = H.conv_grouped_bwd(xd, dzd, wt.detach().to(device).contiguous(), 2, 1, g_)
    assert len(made) == 1 and dx is made[0]
    got_dx, = sync_and_check([dx], [xd, dzd])
    no_nan(dw.cpu(), "grouped wgrad")
    close(dw, wt.grad, torch.float32, "grouped wgrad", extra=30.0)
    close(got_dx, x.grad, dtype, "grouped dgrad")
    # dy_head_grad_split: an fp32 view of nb + nc channels out of nb + ncp
    n, hh, ww, nb, nc, ncp = 3, 13, 11, 64, 10, 16
    gt = torch.randn(n, nb + nc, hh, ww, generator=g)
    gv = V.source(gt, torch.float32, device)
    for sc in (None, torch.tensor(1024.0, device=device)):
        with arena_results(monkeypatch) as made:
            dzb, dzc = H.head_grad_split(gv, nb, nc, ncp, dtype, scale=sc)
        assert len(made) == 2 and dzb is made[0] and dzc is made[1]
        got_b, got_c = sync_and_check([dzb, dzc], [gv])
        f = 1.0 if sc is None else 1024.0
        assert torch.equal(got_b, quantize(gt[:, :nb] * f, dtype)) and torch.equal(got_c[:, :nc], quantize(gt[:, nb:] * f, dtype)) and float(got_c[:, nc:].abs().max()) == 0.0
    # dy_colsum: 10 channels, the tail of the last chunk NaN (the padding only reaches sums that are dropped)
    zq = quantize(torch.randn(3, 10, 17, 19, generator=g), dtype)
    zv = V.source(zq, dtype, device)
    out = H.colsum(zv)
    sync_and_check([], [zv])
    no_nan(out.cpu().view(1, -1, 1, 1), "colsum")
    assert torch.allclose(out.cpu(), zq.sum((0, 2, 3)), rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_maxpool_bwd_and_add_dilated_on_views(dtype, device):
    n, c, h, w, k = 2, 8, 9, 7, 3
    g = torch.Generator().manual_seed(n * 100 + h)
    x = quantize(torch.randint(-3, 4, (n, c, h, w), generator=g).float() * 0.5, dtype).requires_grad_(True)
    go = quantize(torch.randn(n, c, h, w, generator=g), dtype)
    F.max_pool2d(x, k, 1, k // 2).backward(go)
    prev = quantize(torch.randn(n, c, h, w, generator=g), dtype)
    xd, god = V.source(x.detach(), dtype, device, fill=V.BIG_BYTE), V.source(go, dtype, device)  # (a maximum ignores NaN: large values round x)
    gi, gi2 = V.dest((n, c, h, w), dtype, device), V.inout(prev, dtype, device)
    H.maxpool_bwd(xd, god, gi, k, False)
    H.maxpool_bwd(xd, god, gi2, k, True)
    got, got2 = sync_and_check([gi, gi2], [xd, god])
    close(got, x.grad, dtype, "maxpool bwd", extra=4.0)
    close(got2, x.grad + prev, dtype, "maxpool bwd accumulate", extra=4.0)
    # dx[:, :, ::2, ::2] += t on an odd map (test_1x1_stride2_input_gradient_by_scatter's shapes and tolerance)
    b, cc, hh, ww = 2, 64, 21, 27
    prev = quantize(torch.randn(b, cc, hh, ww, generator=g), dtype)
    t = quantize(torch.randn(b, cc, 11, 14, generator=g), dtype)
    dx, tv = V.inout(prev, dtype, device), V.source(t, dtype, device)
    H.add_dilated2_(dx, tv)
    got, = sync_and_check([dx], [tv])
    ref = prev.clone()
    ref[:, :, ::2, ::2] += t
    close(got, ref, dtype, "add_dilated2_", extra=2.0)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_upsample2x_bwd_and_add_nhwc(dtype, device, monkeypatch):
    """The first direct tests of dy_upsample2x_bwd_nhwc (against autograd of the nearest upsample: the sum of each 2 x 2 block) and dy_add_nhwc (a + b):
    fp32 arithmetic on the stored operands, one rounding to the storage type."""
    g = torch.Generator().manual_seed(29)
    n, c, h, w = 2, 16, 5, 7
    x = torch.zeros(n, c, h, w, requires_grad=True)
    gr = quantize(torch.randn(n, c, 2 * h, 2 * w, generator=g), dtype)
    F.interpolate(x, scale_factor=2, mode="nearest").backward(gr)
    gv = V.source(gr, dtype, device)
    with arena_results(monkeypatch) as made:
        dx = H.upsample2x_bwd(gv)
    assert len(made) == 1 and dx is made[0] and tuple(dx.shape) == (n, c, h, w)
    got, = sync_and_check([dx], [gv])
    ref = x.grad.double()
    assert float((got.double() - ref).abs().max()) <= ONE_ROUNDING[dtype] * float(ref.abs().max())
    a, b = quantize(torch.randn(3, 24, 9, 11, generator=g), dtype), quantize(torch.randn(3, 24, 9, 11, generator=g), dtype)
    av, bv, out = V.source(a, dtype, device), V.source(b, dtype, device), V.dest(a.shape, dtype, device)
    H.add_nhwc(av, bv, out=out)
    got, = sync_and_check([out], [av, bv])
    ref = a.double() + b.double()
    assert float((got.double() - ref).abs().max()) <= ONE_ROUNDING[dtype] * float(ref.abs().max())
    # Both entries work in whole 16-byte chunks and have no lane mask for a tail: a channel count that is not whole chunks (10) is refused, and
    # the refused call touches nothing
    t10 = quantize(torch.randn(2, 10, 10, 14, generator=g), dtype)
    g10, a10, o10 = V.source(t10, dtype, device), V.source(t10, dtype, device), V.dest(t10.shape, dtype, device)
    with arena_results(monkeypatch) as made:
        with pytest.raises(H._lib.DyoloError):
            H.upsample2x_bwd(g10)
    with pytest.raises(H._lib.DyoloError):
        H.add_nhwc(a10, g10, out=o10)
    torch.cuda.synchronize()
    for v in (g10, a10, o10, *made):
        V.check_untouched(v, "a view of a refused call")
    assert bool((o10.arena.own == V.NAN_BYTE).all()) and all(bool((v.arena.own == V.NAN_BYTE).all()) for v in made)
