"""Writes (or, with --check, compares against) tests/golden/conv_accepts.json: the eligibility boundaries of the convolution dispatch that
tests/golden/conv_pack_table.json does not reach — what ``PackedConv.for_call`` answers around the view-size, pitch and alignment limits of
the kernels behind DY_WLAYOUT_HALO3X3, and which dense 1x1 stride-1 shapes are packed for the streaming kernel (DY_WLAYOUT_FRAG1X1).

    python tools/make_conv_accepts_golden.py            # record
    python tools/make_conv_accepts_golden.py --check    # compare; exit status 1 on any difference

Needs the built library, no GPU.  Only ``PackedConv``, ``.for_call`` and ``.layout`` are used, so the same script runs on any commit.
One line per key, one character per case:
  ["call", cout, cin, stride, dtype, act]   the pack's layout (R rows, H HALO3X3, F FRAG1X1), and for a HALO3X3 pack "s" (this pack) / "r" (its
                                            rows twin) for every combination of ``call_forms()``, in that order
  ["layout", dtype, for_out_f32, halo, cout]   R / H / F for cin = every whole 16-byte chunk up to 13 K groups of four chunks
"""
from __future__ import annotations

import argparse
import itertools
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from drone_yolo_amd import hip_ops as H  # noqa: E402

TABLE = ROOT / "tests" / "golden" / "conv_accepts.json"
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
# cout, cin, stride of the 3x3 pad-1 layers whose HALO3X3 pack has kernels with preconditions of their own
CALL_SHAPES = [(128, 64, 2), (64, 64, 2), (32, 64, 2), (128, 128, 1), (256, 128, 1), (64, 64, 1), (64, 32, 1), (64, 48, 1)]
COUTS = (4, 8, 16, 20, 32, 64, 68, 128, 256, 512)


def call_forms():
    """(x_bytes, y_bytes, ld_y, y_ptr, residual, out_f32, gathered): both sides of every limit."""
    return itertools.product(((1 << 31) - 1, 1 << 31, (1 << 32) - 65, (1 << 32) - 64), (1 << 20, (1 << 32) - 65, (1 << 32) - 64), (64, 68, 72), (4096, 4104),
                             (False, True), (False, True), (False, True))


def all_keys() -> list:
    keys = []
    for cout, cin, stride in CALL_SHAPES:
        for dt in DTYPES:
            # (128 input channels, stride 1: float16 with an activation and bf16 without are the packs conv_pack_plan gives the layout)
            keys.append(["call", cout, cin, stride, dt, int(not (cin == 128 and dt == "bf16"))])
    keys += [["layout", dt, f32, halo, cout] for dt in DTYPES for f32 in (0, 1) for halo in (None, 0) for cout in COUTS]
    return keys


def _pack(cout, cin, k, stride, dt, act, halo=None, f32=False):
    return H.PackedConv(torch.zeros(cout, cin, k, k), torch.zeros(cout), stride, k // 2, 1, bool(act), DTYPES[dt], "cpu", halo=halo, for_out_f32=bool(f32))


def run_key(key: list) -> str:
    if key[0] == "call":
        _, cout, cin, stride, dt, act = key
        pc = _pack(cout, cin, 3, stride, dt, act)
        out = "RHF"[pc.layout]
        if pc.layout == H._lib.DY_WLAYOUT_HALO3X3:
            for form in call_forms():
                got = pc.for_call(*form)
                assert got is pc or got is pc.rows()
                out += "s" if got is pc else "r"
        return out
    _, dt, f32, halo, cout = key
    e = H.elems_per_chunk(DTYPES[dt])
    return "".join("RHF"[_pack(cout, cin, 1, 1, dt, 1, None if halo is None else bool(halo), f32).layout] for cin in range(e, 13 * 4 * e + 1, e))


def load_table(path=TABLE) -> list:
    with open(path) as f:
        return json.load(f)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--check", action="store_true", help="compare against the committed table instead of writing it")
    ap.add_argument("--table", default=str(TABLE))
    a = ap.parse_args()
    rows = [[key, run_key(key)] for key in all_keys()]
    n = sum(len(r[1]) for r in rows)
    if not a.check:
        with open(a.table, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]\n")
        print(f"wrote {len(rows)} lines, {n} cases to {a.table}")
        return 0
    want = load_table(a.table)
    diff = [(w, r) for w, r in zip(want, rows) if w != r]
    for w, r in diff[:40]:
        print(f"DIFFERS\n  table {w}\n  now   {r}")
    print(f"{len(rows)} lines, {n} cases, {len(diff)} differences against {a.table}")
    return 1 if diff or len(want) != len(rows) else 0


if __name__ == "__main__":
    sys.exit(main())
