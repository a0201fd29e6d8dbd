"""Records tests/golden/stem2_parent.npz: the output bits of dy_stem2_fused for the two small cases of
tests/test_stem2_tiles_gpu.py::test_stem2_parent_bits, fp16 and bf16 (GPU box).

    python tools/make_stem2_golden.py [--lib PATH/libdyolo.so] [--out FILE]

Run it against the library of the commit whose bits are to be kept (``--lib``: another build than drone-yolo_amd/lib); the
file holds data only: per case and dtype the NHWC output as uint16 bit patterns.  Inputs and weights come from the seeds of
``stem2_case`` (the ones of tests/test_kernels_gpu.py::test_fused_stem2_matches_cpu).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(2, 36, 44), (1, 132, 68)]
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}


def stem2_case(shape, dtype):
    """(image, w0, b0, w1, b1) of a case: CPU fp32, weights rounded to the storage type."""
    n, h, w = shape
    g = torch.Generator().manual_seed(h * 3 + w)
    img = torch.rand(n, 3, h, w, generator=g)
    w0 = (torch.randn(32, 3, 3, 3, generator=g) * 0.4).to(dtype).float()
    b0 = torch.randn(32, generator=g) * 0.2
    w1 = (torch.randn(64, 32, 3, 3, generator=g) * (2.0 / 288) ** 0.5).to(dtype).float()
    b1 = torch.randn(64, generator=g) * 0.2
    return img, w0, b0, w1, b1


def key(shape, tag):
    return f"{tag}_{shape[0]}x{shape[1]}x{shape[2]}"


def run_bits(H, shape, dtype, device):
    """The (N, H/4, W/4, 64) output of the fused stem as uint16 bit patterns (numpy)."""
    img, w0, b0, w1, b1 = stem2_case(shape, dtype)
    ps = H.PackedStem2(w0, b0, True, w1, b1, True, dtype, device)
    y = H.stem2_fused(img.to(device), ps)
    torch.cuda.synchronize()
    return y.permute(0, 2, 3, 1).contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "stem2_parent.npz"))
    a = ap.parse_args()
    from drone_yolo_amd import _lib

    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    from drone_yolo_amd import hip_ops as H

    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    arrays = {key(s, t): run_bits(H, s, d, dev) for s in CASES for t, d in DTYPES.items()}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    np.savez_compressed(a.out, **arrays)
    print(f"wrote {a.out}: " + ", ".join(f"{k} {v.shape}" for k, v in arrays.items()) + f" ({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()
