"""Micro-benchmark of dy_detect_branch_fused (conv3x3_hhead) on one Detect level (GPU box).
usage: python tools/bench_branch.py [--lib libdyolo.so] [--batch B] [--dtype fp16|bf16] [--nc 10] [--iters 20] [H ...]   (square maps, 64 channels)"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from drone_yolo_amd import _lib
from drone_yolo_amd import hip_ops as H

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default="", help="another build of libdyolo.so")
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--dtype", default="fp16")
ap.add_argument("--nc", type=int, default=10)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--conf", type=float, default=0.25)
ap.add_argument("sizes", nargs="*", type=int, default=[160, 80])
a = ap.parse_args()
if a.lib:
    _lib.LIB_PATH = os.path.abspath(a.lib)
dt = {"bf16": torch.bfloat16, "fp16": torch.float16}[a.dtype]
dev = torch.device("cuda", 0)
g = torch.Generator().manual_seed(0)
for hh in a.sizes:
    A = hh * hh
    x = torch.randn(a.batch, hh, hh, 64, generator=g).to(dt).to(dev).permute(0, 3, 1, 2)
    pc3 = H.PackedConv(torch.randn(64, 64, 3, 3, generator=g) * (2.0 / 576) ** 0.5, torch.randn(64, generator=g) * 0.2, 1, 1, 1, True, dt, dev)
    pred = torch.zeros((a.batch, 4 + a.nc, A), dtype=torch.float32, device=dev)
    bufs = H.NmsBuffers(a.batch, A, 300, dev)
    for kind, cout in ((1, 64), (2, a.nc)):
        w1, b1 = H.pack_frag1x1(torch.randn(cout, 64, generator=g) * 0.15, torch.randn(cout, generator=g) * 0.3 - (1.6 if kind == 2 else 0.0), dt, dev)

        def run():
            if kind == 2:
                H.nms_reset_counts(bufs)
            H.detect_branch_fused(x, pc3, w1, b1, kind, a.nc, 16, 4.0, pred, 0, nms_bufs=bufs if kind == 2 else None, conf_thres=a.conf)

        run()
        torch.cuda.synchronize()
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.record()
        for _ in range(a.iters):
            run()
        en.record()
        torch.cuda.synchronize()
        us = st.elapsed_time(en) / a.iters * 1e3
        print(f"branch kind {kind} {hh}x{hh} B={a.batch} {a.dtype} nc={a.nc} {H.last_kernel_name():<28s}: {us:8.1f} us")
