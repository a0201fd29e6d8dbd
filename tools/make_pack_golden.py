"""Writes (or, with --check, compares against) tests/golden/conv_pack_table.json: what the weight packers of
drone-yolo_amd/hip_ops.py produce on the CPU — per case the layout and geometry of the pack and one SHA-256 over its bytes.

    python tools/make_pack_golden.py            # record
    python tools/make_pack_golden.py --check    # compare; exit status 1 on any difference

Needs the built library (``PackedConv`` asks it for k_pad / cout_pad), no GPU.  Only the public calls are used (``PackedConv`` and its
``for_call``, ``pack_frag1x1``, ``PackedStem``, ``PackedStem2``, ``PackedC2f``, ``pack_dgrad``, ``set_fp8_act_scale``), so the same script runs
on any commit: a refactor of the packers is right when --check reports no difference before and after it.

A case is a JSON list (``spec``); ``run_case(spec)`` rebuilds its inputs from the spec alone (seeded CPU generator) and returns its record:
layout, k_pad, cout_pad, cin, cout, shape and dtype of ``w``, one SHA-256 over the bytes of ``w``, ``b`` and ``wscale``.  The table has one
line per SHAPE (``table_row``): the key, from which ``group_specs`` lists the shape's cases — which is how tests/test_pack_host.py replays the
table without building the models —, and one SHA-256 over all their records; ``--cases FILE`` writes the records themselves.  Cases:
  conv   every distinct convolution of the five benchmark models (scales n, s, l, x of yolov8-p2-repvgg.yaml and scale n of the -sf YAML at
         nc = 10; the Detect closing 1x1 with for_out_f32, the image layer with cin_pad = 8, the stacked first Detect convolutions), the
         shape lists of the GPU tests (device-vs-host packing, fp8, split float16), in five storage types x halo (None, True, False) x act;
         the 3x3 ones again with DYOLO_HREG_128 / DYOLO_FLAT_K_3X3 off; two with an all-zero output-channel row.  A HALO3X3 pack also
         records what ``for_call`` answers for 2^4 call forms x three input sizes.
  dgrad  the dense ones through ``pack_dgrad`` on CPU weights, stride 1 and 2, no_accumulate both ways
  frag   ``pack_frag1x1`` of every Detect closing 1x1 and every C2f cv1 / cv2
  stem / stem2 / c2f   ``PackedStem``, ``PackedStem2``, ``PackedC2f``
A constructor that refuses a case is recorded as ["raises", <exception type>].
"""
from __future__ import annotations

import argparse
import hashlib
import json
import math
import sys
import zlib
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from drone_yolo_amd import hip_ops as H  # noqa: E402

TABLE = ROOT / "tests" / "golden" / "conv_pack_table.json"
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "fp8": H.FP8, "x2": H.F16X2}
FP8_ACT_SCALE = 0.05
MODELS = [("yolov8-p2-repvgg-sf.yaml", "n"), ("yolov8-p2-repvgg.yaml", "n"), ("yolov8-p2-repvgg.yaml", "s"), ("yolov8-p2-repvgg.yaml", "l"),
          ("yolov8-p2-repvgg.yaml", "x")]
# (cout, cin, k, stride, cin_pad) of tests/test_kernels_gpu.py::test_device_weight_packing_equals_host_packing
DEVICE_PACK_CASES = [(64, 64, 3, 1, None), (48, 40, 3, 1, None), (128, 256, 3, 2, None), (96, 192, 1, 1, None), (20, 100, 1, 1, None), (256, 128, 3, 1, None),
                     (32, 3, 3, 2, 8), (16, 16, 3, 1, None)]
# (cin, cout, k, stride) of tests/test_kernels_gpu.py::test_fp8_conv_matches_dequantised_reference
FP8_CASES = [(64, 64, 3, 1), (160, 80, 1, 1), (80, 160, 3, 2), (640, 320, 1, 1), (96, 48, 3, 1), (160, 160, 3, 1), (320, 320, 3, 1), (400, 160, 1, 1)]
# (cin, cout, k, stride) of tests/test_split_gpu.py::CASES (the first reads the image: 3 channels padded to 8) and (cin, cout) of its grouped cases
SPLIT_CASES = [(32, 64, 3, 2), (64, 64, 3, 1), (96, 64, 1, 1), (768, 512, 1, 1), (256, 256, 3, 1), (512, 64, 3, 1), (16, 24, 3, 1), (24, 48, 1, 1), (128, 128, 3, 2),
               (160, 160, 3, 1), (80, 80, 3, 1), (32, 32, 3, 1), (64, 128, 3, 1), (64, 32, 3, 1)]
SPLIT_GROUPED = [(128, 64), (64, 32), (32, 16), (16, 8), (32, 32), (64, 16)]


def _weights(*shape, zero_row: bool = False):
    """Seeded (by the shape) fp32 weights and bias; ``zero_row``: output channel 1 is all zero (the clamp_min branches of the scales)."""
    g = torch.Generator().manual_seed(zlib.crc32(repr(shape).encode()))
    w = torch.randn(*shape, generator=g) * (2.0 / max(1, shape[1] * shape[2] * shape[3])) ** 0.5
    b = torch.randn(shape[0], generator=g) * 0.2
    if zero_row:
        w[1] = 0
    return w, b


def _digest(*tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        if t is not None:
            h.update(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _name(dt: torch.dtype) -> str:
    return str(dt).replace("torch.", "")


def _pack_record(pc) -> list:
    return [pc.layout, pc.k_pad, pc.cout_pad, pc.cin, pc.cout, list(pc.w.shape), _name(pc.w.dtype), _digest(pc.w, pc.b, pc.wscale)]


def _for_call_record(pc) -> str:
    """"s" (this pack) / "r" (its rows twin) for residual x out_f32 x gathered x misaligned output, at three input sizes."""
    out = ""
    for x_bytes in (1 << 20, 3 << 30, 5 << 30):
        for i in range(16):
            residual, out_f32, gathered, misaligned = bool(i & 1), bool(i & 2), bool(i & 4), bool(i & 8)
            got = pc.for_call(x_bytes, 1 << 20, 60 if misaligned else 64, 4096 + (8 if misaligned else 0), residual, out_f32, gathered)
            out += "s" if got is pc else "r"
            assert got is pc or got is pc.rows()
    return out


def run_case(spec: list) -> list:
    kind = spec[0]
    H.set_fp8_act_scale(FP8_ACT_SCALE)
    hreg, flatk = H.HREG_128[0], H.FLAT_K_3X3[0]
    try:
        if kind == "conv":
            _, cout, cin, k, stride, pad, groups, dt, halo, act, f32, cin_pad, toggles, zero_row = spec
            H.HREG_128[0], H.FLAT_K_3X3[0] = hreg and toggles != "hreg0", flatk and toggles != "flatk0"
            w, b = _weights(cout, cin // groups, k, k, zero_row=bool(zero_row))
            pc = H.PackedConv(w, b, stride, pad, groups, bool(act), DTYPES[dt], "cpu", cin_pad=cin_pad, halo=None if halo is None else bool(halo), for_out_f32=bool(f32))
            return _pack_record(pc) + [_for_call_record(pc) if pc.layout == H._lib.DY_WLAYOUT_HALO3X3 else ""]
        if kind == "dgrad":
            _, cout, cin, k, stride, no_acc, dt = spec
            w, _ = _weights(cout, cin, k, k)
            return _pack_record(H.pack_dgrad(w, stride, DTYPES[dt], "cpu", no_accumulate=bool(no_acc)))
        if kind == "frag":
            _, cout, cin, dt = spec
            w, b = _weights(cout, cin, 1, 1)
            wp, bp = H.pack_frag1x1(w, b, DTYPES[dt], "cpu")
            return [wp.numel(), _name(wp.dtype), bp.numel(), _digest(wp, bp)]
        if kind == "stem":
            _, cout, cin, dt = spec
            ps = H.PackedStem(*_weights(cout, cin, 3, 3), True, DTYPES[dt], "cpu")
            return [ps.w.numel(), _name(ps.w.dtype), ps.b.numel(), _digest(ps.w, ps.b)]
        if kind == "stem2":
            w0, b0 = _weights(32, 3, 3, 3)
            w1, b1 = _weights(64, 32, 3, 3)
            ps = H.PackedStem2(w0, b0, True, w1, b1, True, DTYPES[spec[1]], "cpu")
            return [ps.w1.numel(), _name(ps.w1.dtype), _digest(ps.stem.w, ps.stem.b, ps.w1, ps.b1, ps.w1_scale)]
        if kind == "c2f":
            _, cin, c, cout, cv2_in, dt = spec
            pk = H.PackedC2f(_weights(2 * c, cin, 1, 1), _weights(c, c, 3, 3), _weights(c, c, 3, 3), _weights(cout, cv2_in, 1, 1), True, DTYPES[dt], "cpu")
            return [pk.wa.numel(), pk.w1.numel(), pk.w2.numel(), pk.bias.numel(), _name(pk.wa.dtype), _digest(pk.wa, pk.wb, pk.w1, pk.w2, pk.bias)]
        raise KeyError(kind)
    except (NotImplementedError, ValueError) as e:
        return ["raises", type(e).__name__]
    finally:
        H.HREG_128[0], H.FLAT_K_3X3[0] = hreg, flatk
        H.set_fp8_act_scale(1.0)


def model_shapes():
    """(convs, tails, c2fs) of the five models: convs = {(cout, cin, k, stride, pad, groups, for_out_f32, cin_pad)}, tails / C2f 1x1s =
    {(cout, cin)}, c2fs = {(cin, hidden, cout, cv2 inputs)}."""
    import yaml

    import drone_yolo_amd as D
    from drone_yolo_amd.nn.modules.block import C2f
    from drone_yolo_amd.nn.modules.conv import PlainConv2d
    from drone_yolo_amd.nn.modules.head import Detect

    convs, frags, c2fs = set(), set(), set()
    for name, scale in MODELS:
        d = yaml.safe_load(open(ROOT / "drone-yolo_amd" / "cfg" / "models" / "v8" / name))
        d["scale"], d["nc"] = scale, 10
        model = D.DetectionModel(dict(d), nc=10, verbose=False)
        for m in model.modules():
            if isinstance(m, torch.nn.Conv2d) and m.kernel_size[0] == m.kernel_size[1]:
                image = m.in_channels == 3
                convs.add((m.out_channels, m.in_channels, m.kernel_size[0], m.stride[0], m.padding[0], m.groups, int(isinstance(m, PlainConv2d)), 8 if image else None))
                if isinstance(m, PlainConv2d):
                    frags.add((m.out_channels, m.in_channels))
            if isinstance(m, C2f):
                c1, c2 = m.cv1.conv, m.cv2.conv
                c2fs.add((c1.in_channels, m.c, c2.out_channels, c2.in_channels))
                frags.update({(c1.out_channels, c1.in_channels), (c2.out_channels, c2.in_channels)})
            if isinstance(m, Detect):  # cv2[i][0] and cv3[i][0] stacked along cout (Detect._packed_first)
                for a, b in zip(m.cv2, m.cv3):
                    if isinstance(b[0], torch.nn.Sequential):
                        continue
                    convs.add((a[0].conv.out_channels + b[0].conv.out_channels, a[0].conv.in_channels, 3, 1, 1, 1, 0, None))
    return sorted(convs, key=repr), sorted(frags), sorted(c2fs)


def all_groups() -> list:
    """The table's keys, one per shape: ["conv", cout, cin, k, stride, pad, groups, for_out_f32, cin_pad, zero_row], ["dgrad", cout, cin, k],
    ["frag", cout, cin], ["c2f", cin, hidden, cout, cv2 inputs], ["stem", cout, cin], ["stem2"]."""
    convs, frags, c2fs = model_shapes()
    extra = [(co, ci, k, s, k // 2, 1, 0, cp) for co, ci, k, s, cp in DEVICE_PACK_CASES]
    extra += [(co, ci, k, s, k // 2, 1, 0, None) for ci, co, k, s in FP8_CASES + SPLIT_CASES]
    extra += [(co, ci, 3, 2, 1, math.gcd(ci, co), 0, None) for ci, co in SPLIT_GROUPED] + [(24, 24, 3, 2, 1, 8, 0, None)]
    shapes = convs + [s for s in sorted(set(extra), key=repr) if s not in convs]
    keys = [["conv", *s, 0] for s in shapes] + [["conv", 64, 64, 3, 1, 1, 1, 0, None, 1], ["conv", 96, 192, 1, 1, 0, 1, 0, None, 1]]
    keys += [["dgrad", *t] for t in sorted({(cout, cin, k) for cout, cin, k, _, _, g, _, _ in shapes if g == 1})]
    keys += [["frag", *t] for t in frags] + [["c2f", *t] for t in c2fs] + [["stem", *t] for t in ((32, 3), (16, 3), (64, 1), (80, 3))] + [["stem2"]]
    return keys


def group_specs(key: list) -> list:
    """The cases of one shape (specs for ``run_case``), from the key alone."""
    kind = key[0]
    if kind == "conv":
        cout, cin, k, s, p, g, f32, cin_pad, zero_row = key[1:]
        if zero_row:
            return [["conv", cout, cin, k, s, p, g, dt, None, 1, f32, cin_pad, "", 1] for dt in DTYPES]
        specs = []
        for dt in DTYPES:
            # (fp8 and split float16 have the row layout only: neither halo nor act reaches their packs, three of the six combinations pin that)
            for halo, act in ((None, 1), (1, 0), (0, 1)) if dt in ("fp8", "x2") else ((h, a) for h in (None, 1, 0) for a in (1, 0)):
                specs.append(["conv", cout, cin, k, s, p, g, dt, halo, act, f32, cin_pad, "", 0])
            if k == 3 and g == 1 and dt in ("bf16", "f16"):
                specs += [["conv", cout, cin, k, s, p, g, dt, None, act, f32, cin_pad, toggles, 0] for toggles in ("hreg0", "flatk0") for act in (1, 0)]
        return specs
    if kind == "dgrad":
        # the training storage types; fp8 and split float16 (the host route only) for the shapes of the device-vs-host packing test
        dts = DTYPES if tuple(key[1:]) in [c[:3] for c in DEVICE_PACK_CASES] else ("f32", "bf16", "f16")
        return [["dgrad", *key[1:], s, na, dt] for dt in dts for s in (1, 2) for na in (0, 1)]
    if kind in ("frag", "c2f"):
        return [[*key, dt] for dt in ("bf16", "f16", "f32", "x2")]
    return [[*key, dt] for dt in (DTYPES if kind == "stem" else ("f16", "x2"))]


def run_group(key: list) -> list:
    """[(spec, result)] of one shape."""
    return [[spec, run_case(spec)] for spec in group_specs(key)]


def table_row(key: list, pairs: list) -> list:
    """The line of the table: key, case count, the default layouts (conv: halo None, act on, per storage type in DTYPES order — R rows,
    H HALO3X3, F FRAG1X1, - refused) and one SHA-256 over the JSON of all (spec, result) pairs of the shape."""
    marks = "".join("-" if r[0] == "raises" else "RHF"[r[0]] for s, r in pairs if key[0] == "conv" and s[8] is None and s[9] == 1 and s[12] == "")
    return [key, len(pairs), marks, hashlib.sha256(json.dumps(pairs, separators=(",", ":")).encode()).hexdigest()]


def load_table(path=TABLE) -> list:
    with open(path) as f:
        return json.load(f)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--check", action="store_true", help="compare against the committed table instead of writing it")
    ap.add_argument("--table", default=str(TABLE))
    ap.add_argument("--cases", default="", metavar="FILE", help="also write every (spec, result) pair, one per line: diff two commits' files to find the case behind a differing line")
    a = ap.parse_args()
    groups = [(key, run_group(key)) for key in all_groups()]
    rows = [table_row(key, pairs) for key, pairs in groups]
    if a.cases:
        with open(a.cases, "w") as f:
            f.writelines(json.dumps(pair, separators=(",", ":")) + "\n" for _, pairs in groups for pair in pairs)
    n = sum(r[1] for r in rows)
    if not a.check:
        with open(a.table, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]\n")
        print(f"wrote {len(rows)} shapes, {n} cases to {a.table}")
        return 0
    want = {json.dumps(r[0]): r for r in load_table(a.table)}
    got = {json.dumps(r[0]): r for r in rows}
    diff = [k for k in sorted(set(want) | set(got)) if want.get(k) != got.get(k)]
    for k in diff[:40]:
        print(f"DIFFERS {k}\n  table {want.get(k)}\n  now   {got.get(k)}")
    print(f"{len(rows)} shapes, {n} cases, {len(diff)} differences against {a.table}")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
