"""Writes (or, with --check, compares against) tests/golden/conv_dispatch.json: which kernel ``dy_conv2d_nhwc`` runs for a call and what it
computes — per case ``last_kernel_name()``, ``conv_stats_written()`` and one SHA-256 over the output bytes.  Needs an MI355X.

    python tools/make_conv_dispatch_golden.py            # record
    python tools/make_conv_dispatch_golden.py --check    # compare; exit status 1 on any difference

Only public calls are used (``PackedConv``, ``conv2d``, ``BnState``, ``to_nhwc`` / ``to_nchw_f32``, ``set_fp8_act_scale``), so the same script runs
on any commit: a refactor of the dispatch is right when --check reports no difference before and after it.  Every case is ONE ``conv2d``
launch on inputs from a CPU generator seeded by the case; no kernel on the route to ``y`` adds into ``y`` atomically, so the bytes repeat.

A case is a JSON list ``[tag, dtype, cin, cout, k, stride, B, H, W, act, halo, form]``; ``run_case`` rebuilds everything from it.  Forms:
  plain / residual / out_f32 / unaligned (output pitch cout + 4) / x2 (two sources of cin / 2) / up2x (source at half size)
  stats    ``bn_stats``: the filled workspace slots are hashed behind ``y``;  stats_y: likewise, ``y`` alone (atomic slots: order-dependent sums)
  dil2     the zero-dilated gather of a stride-2 input gradient (source at half size)
  to_f16 / to_fp8   ``out_dtype`` (fp8 in -> float16 out, float16 in -> fp8 out)
A call that is refused is recorded as ["raises", <exception type>].
"""
from __future__ import annotations

import argparse
import hashlib
import json
import sys
import zlib
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from drone_yolo_amd import hip_ops as H  # noqa: E402

TABLE = ROOT / "tests" / "golden" / "conv_dispatch.json"
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "fp8": H.FP8, "x2": H.F16X2}
FP8_ACT_SCALE = 0.05
PLAIN3, BITS16 = ("f32", "bf16", "f16"), ("bf16", "f16")

# the rows of tests/test_kernels_gpu.py::CONV_CASES with B * H * W <= 2 * 40 * 40: cin, cout, k, s, B, H, W, act, tag
BASE = [
    (32, 64, 3, 2, 2, 40, 40, True, "repvgg-like s2"), (64, 64, 3, 1, 2, 40, 40, True, "3x3 s1 BN=64"), (32, 32, 3, 1, 1, 24, 20, True, "3x3 s1 BN=32"),
    (96, 64, 1, 1, 2, 40, 40, True, "1x1 K=96 (K tail)"), (768, 512, 1, 1, 2, 20, 20, True, "1x1 wide"), (256, 256, 3, 1, 1, 20, 20, True, "3x3 deep small-M"),
    (64, 64, 3, 1, 1, 13, 17, True, "odd spatial (M tail)"), (16, 24, 3, 1, 1, 12, 12, True, "n-scale odd cout"), (24, 48, 1, 1, 1, 12, 12, True, "cin=24"),
    (48, 64, 3, 1, 2, 33, 37, True, "halo cin=48 odd dims"), (128, 128, 3, 2, 2, 40, 40, True, "halo s2 deep"),
    (384, 128, 1, 1, 2, 40, 40, True, "1x1 stream 384->128 (12 k-groups)"),
    (256, 256, 1, 1, 2, 40, 40, True, "1x1 stream 256->256 (2 n-tiles)"), (128, 128, 1, 1, 1, 13, 11, True, "1x1 stream odd M tail"),
    (64, 8, 1, 1, 1, 20, 20, False, "1x1 stream cout=8 (NF=1)"), (64, 64, 3, 2, 2, 40, 36, True, "hreg s2 64->64"),
    (64, 128, 3, 2, 3, 33, 31, True, "hreg s2 64->128 odd dims"), (64, 64, 3, 2, 1, 8, 8, False, "hreg s2 tiny no act"),
    (128, 128, 3, 1, 2, 40, 40, True, "hreg 128->128 (four chunks in registers)"), (128, 64, 3, 1, 3, 33, 31, True, "hreg 128->64 odd dims"),
    (128, 256, 3, 1, 1, 8, 16, False, "hreg 128->256 tiny no act"),
]
# tile choices that depend on the tile count
TILES = [(32, 32, 3, 1, 8, 160, 160, True, "large M BN=32"), (64, 64, 3, 1, 40, 40, 40, True, "halo many tiles per block")]
# flat-K tile widths 80 / 160 / 160 x 2 / 80 (1x1)
FLATK = [(80, 80, 3, 1), (160, 160, 3, 1), (320, 320, 3, 1), (160, 80, 1, 1)]
# the shapes whose call forms are swept: the three with a HALO3X3 pack whose kernels refuse some, and one deep layer on the rows layout
FORM_SHAPES = [(64, 128, 3, 2, "64->128 s2"), (128, 128, 3, 1, "128->128 s1"), (64, 64, 3, 1, "64->64 s1"), (256, 256, 3, 1, "256->256 deep")]
FORMS = ("plain", "residual", "out_f32", "unaligned", "x2", "up2x")
# one shape per kernel family with a statistics epilogue: cin, cout, k, s, B, H, W, tag
STATS = [(64, 64, 3, 1, 2, 24, 20, "hreg"), (64, 128, 3, 2, 2, 24, 20, "hreg_s2"), (32, 32, 3, 1, 2, 24, 20, "halo"), (64, 64, 1, 1, 2, 24, 20, "1x1 stream"),
         (512, 256, 1, 1, 2, 20, 20, "glds"), (160, 160, 3, 1, 2, 24, 20, "flat-K")]


def all_cases() -> list:
    c = [[tag, dt, ci, co, k, s, b, h, w, int(act), None, "plain"] for ci, co, k, s, b, h, w, act, tag in BASE + TILES for dt in PLAIN3]
    # M * Cout = 256 * 256 * 512: the 256 x 256 tile of the LDS-DMA GEMM (the rows layout: the default pack of this 1x1 is the streaming kernel's)
    c += [["glds 256x256 tile", "bf16", 256, 256, 1, 1, 8, 128, 128, 1, 0, "plain"]]
    c += [[f"flat-K {ci}->{co}", dt, ci, co, k, s, 1, 20, 20, 1, None, "plain"] for ci, co, k, s in FLATK for dt in BITS16]
    # (a bf16 128 -> 128 pack WITH an activation stays on the rows layout: conv_pack_plan, r05)
    c += [[f"{tag} {form}", dt, ci, co, k, s, 2, 24, 20, int(not (ci == 128 and dt == "bf16")), None, form]
          for ci, co, k, s, tag in FORM_SHAPES for dt in BITS16 for form in FORMS]
    c += [[f"stats {tag}", dt, ci, co, k, s, b, h, w, 0, None, "stats"] for ci, co, k, s, b, h, w, tag in STATS for dt in BITS16]
    # 3 * 212 * 212 output pixels: 1,054 row blocks of 128, more than the workspace has slots
    c += [["stats atomic slots", "bf16", 32, 64, 1, 2, 3, 424, 424, 0, None, "stats_y"]]
    c += [[f"{tag} dil2", dt, ci, co, k, 1, 2, 24, 20, 0, None, "dil2"] for ci, co, k, s, tag in FORM_SHAPES[1:] for dt in BITS16]
    for ci, co, k, s in ((160, 80, 1, 1), (160, 160, 3, 1)):
        c += [[f"fp8 {ci}->{co}", "fp8", ci, co, k, s, 1, 20, 20, 1, None, "plain"], [f"fp8 -> f16 {ci}->{co}", "fp8", ci, co, k, s, 1, 20, 20, 1, None, "to_f16"],
              [f"f16 -> fp8 {ci}->{co}", "f16", ci, co, k, s, 1, 20, 20, 1, 0, "to_fp8"]]
    c += [["split 32->32 hsplit", "x2", 32, 32, 3, 1, 1, 64, 56, 1, None, "plain"], ["split 64->64 hsplit", "x2", 64, 64, 3, 1, 1, 64, 56, 1, None, "plain"],
          ["split 64->64 flat-K", "x2", 64, 64, 3, 1, 1, 20, 20, 1, None, "plain"], ["split 1x1 96->64", "x2", 96, 64, 1, 1, 1, 20, 20, 1, None, "plain"]]
    # groups = gcd(cin, cout): conv_smallgroup_kernel, conv_smallgroup_split_kernel, and the generic grouped kernel (cout 12: no whole chunks)
    c += [["grouped 16->8 s2", "bf16", 16, 8, 3, 2, 1, 20, 20, 1, None, "grouped"], ["grouped split 16->8 s2", "x2", 16, 8, 3, 2, 1, 20, 20, 1, None, "grouped"],
          ["grouped 24->12 s2", "bf16", 24, 12, 3, 2, 1, 20, 20, 1, None, "grouped"]]
    return c


def _dev(t: torch.Tensor, dtype: torch.dtype, device, ld=None) -> torch.Tensor:
    """CPU NCHW fp32 -> device NHWC view in ``dtype`` (pixel pitch ``ld``)."""
    if dtype == H.F16X2:
        return H.to_nhwc(t.to(device).contiguous(), dtype, c_pad=-(-t.shape[1] // 8) * 8)
    n, c, h, w = t.shape
    buf = torch.zeros((n, h, w, ld or c), dtype=dtype).to(device)
    buf[..., :c] = t.permute(0, 2, 3, 1).contiguous().to(dtype).to(device)
    return buf.permute(0, 3, 1, 2)[:, :c]


def _bytes(t: torch.Tensor) -> bytes:
    t = H.to_nchw_f32(t).cpu() if t.dtype == H.F16X2 else t.detach().cpu().permute(0, 2, 3, 1)
    return t.contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()


def run_case(spec: list, device) -> list:
    import math

    tag, dt, cin, cout, k, s, b, h, w, act, halo, form = spec
    dtype = DTYPES[dt]
    g = torch.Generator().manual_seed(zlib.crc32(json.dumps(spec).encode()))
    groups = math.gcd(cin, cout) if form == "grouped" else 1
    wt = torch.randn(cout, cin // groups, k, k, generator=g) * (2.0 / (cin // groups * k * k)) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.2
    half = form in ("up2x", "dil2")
    x = torch.randn(b, cin, h // 2 if half else h, w // 2 if half else w, generator=g)
    ho, wo = H.conv_out_hw(h, w, k, s, k // 2)
    r = torch.randn(b, cout, ho, wo, generator=g)
    if dt == "fp8":
        x, r = x * 1.5 / FP8_ACT_SCALE, r / FP8_ACT_SCALE
    H.set_fp8_act_scale(FP8_ACT_SCALE)
    try:
        pc = H.PackedConv(wt, bias, s, k // 2, groups, bool(act), dtype, device, halo=None if halo is None else bool(halo))
        kw, state = {}, None
        if form == "x2":
            xin, kw = _dev(x[:, : cin // 2], dtype, device), {"x2": _dev(x[:, cin // 2:], dtype, device)}
        else:
            xin = _dev(x, dtype, device)
        if form == "residual":
            kw = {"residual": _dev(r, dtype, device)}
        elif form == "out_f32":
            kw = {"out_f32": True}
        elif form == "unaligned":
            kw = {"out": _dev(torch.zeros(b, cout, ho, wo), dtype, device, ld=cout + 4)}
        elif form == "up2x":
            kw = {"up2x": True}
        elif form == "dil2":
            kw = {"dil2": True}
        elif form in ("stats", "stats_y"):
            state = H.BnState(cout, device)
            state.ws.zero_()
            kw = {"bn_stats": state}
        elif form == "to_f16":
            kw = {"out_dtype": torch.float16}
        elif form == "to_fp8":
            kw = {"out_dtype": H.FP8}
        y = H.conv2d(xin, pc, **kw)
        name, slots = H.last_kernel_name(), H.conv_stats_written()
        torch.cuda.synchronize()
        sha = hashlib.sha256(_bytes(y))
        if form == "stats":
            sha.update(state.ws[2 * cout * 8: (1 + slots) * 2 * cout * 8].cpu().numpy().tobytes())
        return [name, slots, sha.hexdigest()]
    except (H._lib.DyoloError, NotImplementedError) as e:  # the library refuses the call / the plan refuses the pack; anything else ends the run
        return ["raises", type(e).__name__]
    finally:
        H.set_fp8_act_scale(1.0)


def load_table(path=TABLE) -> list:
    with open(path) as f:
        return json.load(f)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--check", action="store_true", help="compare against the committed table instead of writing it")
    ap.add_argument("--table", default=str(TABLE))
    a = ap.parse_args()
    device = torch.device("cuda", 0)
    rows = [[spec, run_case(spec, device)] for spec in all_cases()]
    if not a.check:
        with open(a.table, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]\n")
        print(f"wrote {len(rows)} cases to {a.table}")
        return 0
    want = load_table(a.table)
    diff = [(w_, r) for w_, r in zip(want, rows) if w_ != r]
    for w_, r in diff[:40]:
        print(f"DIFFERS\n  table {w_}\n  now   {r}")
    print(f"{len(rows)} cases, {len(diff)} differences against {a.table}")
    return 1 if diff or len(want) != len(rows) else 0


if __name__ == "__main__":
    sys.exit(main())
