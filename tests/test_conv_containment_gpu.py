"""``dy_conv2d_nhwc`` on strided views, every dispatch leaf: the cases of tests/golden/conv_dispatch.json (tools/make_conv_dispatch_golden.py: same
seed, packs and keywords) with every operand carved out of an arena (tests/_view_util.py) — sources as channel slices at 16 bytes of a pitch 32 bytes
wider than their channels, all bytes around them NaN; the output as a slice at 32 bytes of a pitch 64 bytes wider, 0xA5 around it and NaN inside.

Per case: (a) the result against a float64 ``F.conv2d`` on the dtype-rounded operands, to the tolerances of the parity tests; (b) no NaN in it (a
guard byte was consumed, or an element never stored); (c) no byte of the output arena outside the view changed; (d) no byte of any source arena
changed; (e) the kernel that ran and the statistics slots it reported are the table's, so the sweep runs the kernel the table names."""
import collections
import importlib.util
import json
import math
import os
import zlib

import pytest
import torch
import torch.nn.functional as F

from tests import _view_util as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_conv_dispatch_golden", os.path.join(ROOT, "tools", "make_conv_dispatch_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
H = G.H
TABLE = G.load_table()

MAX_PIXELS = 4000
BIG = "conv_gemm_glds_kernel<256,256>"  # its only case has 131,072 pixels: swept too (the float64 reference of a 1x1 takes about a second)
SWEPT = [row for row in TABLE if row[0][6] * row[0][7] * row[0][8] <= MAX_PIXELS or row[1][0] == BIG]
IDS = [f"{row[0][0]}-{row[0][1]}" for row in SWEPT]

# Cases where an aligned slice view makes the dispatcher take another kernel than the contiguous call of the table did:
# "<tag>-<dtype>": (kernel observed, statistics slots observed, the routing rule that decides it).
# None observed: the routing rules that look at a view (dy_conv3x3_halo_route: ld_y % 8, y % 16, view sizes below 2 / 4 GiB; the 16-byte tests of the
# other dispatchers) ask for 16-byte alignment and a size, which an aligned slice keeps; no rule asks for ld == c.
OTHER_ON_A_SLICE = {
}


def _key(spec):
    return f"{spec[0]}-{spec[1]}"


def expected_kernel(spec, want):
    return OTHER_ON_A_SLICE[_key(spec)][:2] if _key(spec) in OTHER_ON_A_SLICE else (want[0], want[1])


def test_every_kernel_of_the_table_is_swept():
    """Computed from the table and OTHER_ON_A_SLICE: every distinct kernel name of the table is reached by at least one swept case."""
    names = {want[0] for _, want in TABLE if want[0] != "raises"}
    reached = collections.Counter(expected_kernel(spec, want)[0] for spec, want in SWEPT if want[0] != "raises")
    small = collections.Counter(expected_kernel(spec, want)[0] for spec, want in SWEPT if want[0] != "raises" and spec[6] * spec[7] * spec[8] <= MAX_PIXELS)
    assert names - set(reached) == set(), sorted(names - set(reached))
    assert names - set(small) <= {BIG}  # the one name without a small case
    assert set(OTHER_ON_A_SLICE) <= {_key(spec) for spec, _ in SWEPT}
    assert any(want[0] == "raises" for _, want in SWEPT)
    forms = {spec[-1] for spec, _ in SWEPT}
    assert forms >= {"plain", "residual", "out_f32", "unaligned", "x2", "up2x", "dil2", "stats", "to_f16", "to_fp8", "grouped"} and any(s[1] == "x2" for s, _ in SWEPT)


def source(t, dtype, device):
    """CPU fp32 NCHW values -> a sealed "in" arena view on the device: slice at 16 bytes, pitch = channels + 32 bytes."""
    if dtype != H.F16X2:
        return V.source(t, dtype, device)
    n, c, h, w = t.shape
    c = -(-c // 8) * 8
    v = V.carve((n, c, h, w), dtype, device, 16, c * 4 + 32, "in")
    H.to_nhwc(t.to(device).contiguous(), dtype, c_pad=c, out=v)  # the project's own splitter: the bytes the table's run had
    torch.cuda.synchronize()
    v.arena.seal()
    return v


def dest(shape, dtype, device, unaligned=False):
    if unaligned:  # the table's form: pitch cout + 4 elements, no 16-byte rows
        return V.carve(shape, dtype, device, 0, (shape[1] + 4) * V.ESIZE[dtype], "out", aligned=False)
    return V.dest(shape, dtype, device)  # slice at 32 bytes, pitch = channels + 64 bytes


def reference(spec, wt, bias, x, r, groups):
    """float64 convolution on the operands as the device holds them, activation, then the residual."""
    tag, dt, cin, cout, k, s, b, h, w, act, halo, form = spec
    dtype = G.DTYPES[dt]
    if dt == "fp8":  # e4m3fn quanta at the activation scale; weights quantised per output channel (test_fp8_conv_matches_dequantised_reference)
        xr = x.to(H.FP8).double() * G.FP8_ACT_SCALE
        ws = (wt.reshape(cout, -1).abs().amax(1) / 448.0).clamp_min(1e-12).view(-1, 1, 1, 1)
        wr = ((wt / ws).to(H.FP8).float() * ws).double()
    elif dt == "x2":  # 22 bits of each operand: inside the type's own tolerance
        xr, wr = x.double(), wt.double()
    else:
        xr, wr = V.rounded(x, dtype).double(), V.rounded(wt, dtype).double()
    if form == "up2x":
        xr = F.interpolate(xr, scale_factor=2, mode="nearest")
    elif form == "dil2":
        z = torch.zeros(b, cin, h, w, dtype=torch.float64)
        z[:, :, ::2, ::2] = xr
        xr = z
    y = F.conv2d(xr, wr, bias.double(), s, k // 2, groups=groups)
    if act:
        y = F.silu(y)
    if form == "residual":
        y = y + (r.to(H.FP8).double() * G.FP8_ACT_SCALE if dt == "fp8" else r.double() if dt == "x2" else V.rounded(r, dtype).double())
    return y


def check_result(spec, got, ref, odt):
    """(a), with the bars of the parity tests: RTOL and the residual's extra = 2 of tests/test_kernels_gpu.py::check_close, 4e-6 of the output
    scale for split float16 (tests/test_split_gpu.py), and for fp8 those of test_fp8_conv_matches_dequantised_reference."""
    from tests.test_kernels_gpu import RTOL

    dt, form = spec[1], spec[-1]
    scale = max(float(ref.abs().max()), 1e-6)
    if odt == H.FP8:  # ``got`` in quanta: the reference rounded to e4m3 at the activation scale, one quantum where the sums straddle a boundary (<= 2 %)
        want_q = (ref.float() / G.FP8_ACT_SCALE).clamp(-448, 448).to(H.FP8).float()
        diff = (got - want_q).abs()
        step = want_q.abs().clamp_min(2.0 ** -6) * 0.126
        print(f"   fp8: worst diff / step {float((diff / step).max()):.4f}, fraction off {float((diff > 0).float().mean()):.4f}")
        assert bool((diff <= step).all()), float((diff / step).max())
        assert float((diff > 0).float().mean()) <= 0.02
        return
    err = float((got.double() - ref).abs().max())
    print(f"{_key(spec)}: max|err| {err:.4e}, output scale {scale:.4f}")
    if dt == "x2":
        assert err <= 4e-6 * scale, (err, scale)
    elif dt == "fp8":  # fp8 -> float16: the fp32 result rounded once to float16
        assert odt == torch.float16 and err <= RTOL[torch.float16] * scale, (err, scale)
    else:
        tol = RTOL[G.DTYPES[dt]] * (2.0 if form == "residual" else 1.0) * scale
        assert err <= tol, f"max|err| {err:.4e} vs scale {scale:.3f} (tol {tol:.4e})"


@pytest.mark.gpu
@pytest.mark.parametrize("spec,want", SWEPT, ids=IDS)
def test_conv_on_views_is_right_and_contained(spec, want, device):
    tag, dt, cin, cout, k, s, b, h, w, act, halo, form = spec
    dtype = G.DTYPES[dt]
    g = torch.Generator().manual_seed(zlib.crc32(json.dumps(spec).encode()))
    groups = math.gcd(cin, cout) if form == "grouped" else 1
    wt = torch.randn(cout, cin // groups, k, k, generator=g) * (2.0 / (cin // groups * k * k)) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.2
    half = form in ("up2x", "dil2")
    x = torch.randn(b, cin, h // 2 if half else h, w // 2 if half else w, generator=g)
    ho, wo = H.conv_out_hw(h, w, k, s, k // 2)
    r = torch.randn(b, cout, ho, wo, generator=g)
    if dt == "fp8":
        x, r = x * 1.5 / G.FP8_ACT_SCALE, r / G.FP8_ACT_SCALE
    odt = torch.float32 if form == "out_f32" else torch.float16 if form == "to_f16" else H.FP8 if form == "to_fp8" else dtype
    H.set_fp8_act_scale(G.FP8_ACT_SCALE)
    try:
        pc = H.PackedConv(wt, bias, s, k // 2, groups, bool(act), dtype, device, halo=None if halo is None else bool(halo))
        sources, kw, state = [], {}, None
        if form == "x2":
            xin, x2 = source(x[:, : cin // 2], dtype, device), source(x[:, cin // 2:], dtype, device)
            sources, kw = [xin, x2], {"x2": x2}
        else:
            xin = source(x, dtype, device)
            sources = [xin]
        if form == "residual":
            sources.append(source(r, dtype, device))
            kw = {"residual": sources[-1]}
        elif form == "out_f32":
            kw = {"out_f32": True}
        elif form == "up2x":
            kw = {"up2x": True}
        elif form == "dil2":
            kw = {"dil2": True}
        elif form in ("stats", "stats_y"):
            state = H.BnState(cout, device)
            state.ws.fill_(V.OUT_GUARD_BYTE)
            kw = {"bn_stats": state}
        elif form == "to_f16":
            kw = {"out_dtype": torch.float16}
        elif form == "to_fp8":
            kw = {"out_dtype": H.FP8}
        y = dest((b, cout, ho, wo), odt, device, unaligned=form == "unaligned")
        if want[0] == "raises":
            with pytest.raises({"DyoloError": H._lib.DyoloError, "NotImplementedError": NotImplementedError}[want[1]]):
                H.conv2d(xin, pc, out=y, **kw)
            torch.cuda.synchronize()
            V.check_untouched(y, "output of a refused call")
            assert bool((y.arena.own == V.NAN_BYTE).all())
            for i, v in enumerate(sources):
                V.check_untouched(v, f"source {i} of a refused call")
            return
        H.conv2d(xin, pc, out=y, **kw)
        name, slots = H.last_kernel_name(), H.conv_stats_written()
        torch.cuda.synchronize()
    finally:
        H.set_fp8_act_scale(1.0)
    print(f"{_key(spec)}: ran {name}, {slots} statistics slots (table: {want[0]}, {want[1]})")
    # (c), (d): containment first — a stray store says more than the wrong number it may also cause
    V.check_untouched(y, f"output arena ({name})")
    for i, v in enumerate(sources):
        V.check_untouched(v, f"source arena {i} ({name})")
    if state is not None:
        behind = state.ws[(1 + slots) * 2 * cout * 8:]
        assert bool((behind == V.OUT_GUARD_BYTE).all()), f"{name}: the workspace behind its {slots} slots was written"
    # (b), (a)
    got = V.read(y).cpu()
    V.check_no_nan(y, got, f"output ({name})")
    check_result(spec, got, reference(spec, wt, bias, x, r, groups), odt)
    if state is not None and slots > 0:
        # the slots that were written hold per-channel partial sums and sums of squares of the STORED output (the bar of
        # tests/test_train_gpu.py::test_conv_epilogue_batchnorm_statistics): a guard row or channel folded into them shows here, not in y
        part = state.ws.view(torch.float64)[2 * cout: (1 + slots) * 2 * cout].view(slots, 2 * cout).sum(0).cpu()
        assert bool(torch.isfinite(part).all()), f"{name}: a statistics slot is not finite"
        gd = got.double()
        sums = torch.cat([gd.sum((0, 2, 3)), (gd * gd).sum((0, 2, 3))])
        print(f"   stats: max|err| {float((part - sums).abs().max()):.4e}, scale {float(sums.abs().max()):.4f}")
        assert float((part - sums).abs().max()) <= 2e-5 * float(sums.abs().max()), f"{name}: the statistics slots do not hold the sums of y"
    # (e)
    assert (name, slots) == tuple(expected_kernel(spec, want)), f"{_key(spec)}: ran {name} with {slots} slots, the table has {want[0]} with {want[1]}"
