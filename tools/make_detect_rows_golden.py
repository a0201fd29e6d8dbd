"""Records tests/golden/detect_rows_parent.npz: the output bits of the three Detect decode kernels (dy_detect_decode and
dy_detect_head_decode for f32 / bf16 / f16 / split float16) with the fused candidate filter, for the cases of
tests/test_detect_rows_gpu.py (GPU box).

    python tools/make_detect_rows_golden.py [--lib PATH/libdyolo.so] [--out FILE]

Run it against the library of the commit whose bits are to be kept (``--lib``: another build than drone-yolo_amd/lib).  The file
holds outputs only; the inputs come from the seeds of ``case_inputs``.  Per case:
    <case>_pred    the decoded (N, 4 + nc, A) fp32 tensor as its four byte planes, uint8 (4, N * (4 + nc) * A): byte k of every
                   value in plane k (deflate packs the sign / exponent plane that way; ``planes`` / ``unplanes`` convert)
    <case>_counts  candidates per image, int32 (N,)
    <case>_keys    every image's keys in ascending order, images concatenated, uint64
    <case>_cls     the class stored for the anchor of each of those keys, uint16
The append order of the candidates is not deterministic, hence the sort.

Batch 1: with batch 2 the file is twice the size of the largest ``*_parent.npz`` beside it (``save_npz`` on what is left).  nc 1 runs once (dy_detect_decode).
"""
import argparse
import ctypes
import functools
import io
import os
import sys
import zipfile

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH = 1
SHAPES = [(23, 25), (5, 7), (1, 1)]  # 575 anchors: nine 64-anchor tiles, the last ragged, two workgroup groups of the head kernel; 35 (< 64); 1
STRIDES = [8.0, 16.0, 32.0]
ANCHORS = sum(h * w for h, w in SHAPES)
CONF = 0.9  # about a fifth of the anchors clear it
MASKED_CLASS = 3  # the nc 10 cases run with a class mask that removes this class
KERNELS = ["decode", "head_f32", "head_bf16", "head_f16", "head_split"]
CASES = [(k, 10) for k in KERNELS] + [("decode", 1)]


def case_name(kernel, nc):
    return f"{kernel}_nc{nc}"


def head_dtype(kernel, H):
    return {"head_f32": torch.float32, "head_bf16": torch.bfloat16, "head_f16": torch.float16, "head_split": H.F16X2}[kernel]


@functools.lru_cache(maxsize=None)
def case_inputs(kernel, nc):
    """CPU fp32 inputs of a case and the fp32 logits (N, 64 + nc, h, w) per level they stand for (the oracle's input).
    decode: the logits themselves.  head_*: the two branch inputs (64 channels each), 1x1 weights and biases, operands rounded to the
    storage type (split float16 keeps fp32 operands: 22 significant bits)."""
    g = torch.Generator().manual_seed(1000 * KERNELS.index(kernel) + nc)
    if kernel == "decode":
        feats = [torch.randn(BATCH, 64 + nc, h, w, generator=g) * 2.5 for h, w in SHAPES]
        for f in feats:
            f[:, 64:] -= 3.0  # class logits around -3, as a trained head's
        return dict(feats=feats)
    dt = {"head_f32": torch.float32, "head_bf16": torch.bfloat16, "head_f16": torch.float16, "head_split": torch.float32}[kernel]
    rnd = lambda t: t.to(dt).float()
    xb = [rnd(torch.randn(BATCH, 64, h, w, generator=g)) for h, w in SHAPES]
    xc = [rnd(torch.randn(BATCH, 64, h, w, generator=g)) for h, w in SHAPES]
    wb = [rnd(torch.randn(64, 64, 1, 1, generator=g) * 0.25) for _ in SHAPES]
    wc = [rnd(torch.randn(nc, 64, 1, 1, generator=g) * 0.2) for _ in SHAPES]
    bb = [torch.randn(64, generator=g) for _ in SHAPES]
    bc = [torch.randn(nc, generator=g) - 1.0 for _ in SHAPES]
    feats = [torch.cat([F.conv2d(xb[i].double(), wb[i].double(), bb[i].double()), F.conv2d(xc[i].double(), wc[i].double(), bc[i].double())], 1).float()
             for i in range(len(SHAPES))]
    return dict(feats=feats, xb=xb, xc=xc, wb=wb, wc=wc, bb=bb, bc=bc)


def class_mask(nc):
    """uint8 (nc,) with MASKED_CLASS removed for nc 10; None for nc 1."""
    if nc == 1:
        return None
    m = torch.ones(nc, dtype=torch.uint8)
    m[MASKED_CLASS] = 0
    return m


def oracle_candidates(kernel, nc):
    """Per image: (anchors whose best class clears CONF, those of them the class mask keeps), from the oracle's decode on the CPU."""
    from oracle import drone_yolo_oracle as O

    y = O.detect_decode(case_inputs(kernel, nc)["feats"], STRIDES, nc)
    best, j = y[:, 4:].max(1)
    above = best > CONF
    m = class_mask(nc)
    kept = above if m is None else above & m.bool()[j]
    return above.sum(1).tolist(), kept.sum(1).tolist()


def planes(a):
    return np.ascontiguousarray(np.ascontiguousarray(a, dtype=np.float32).view(np.uint8).reshape(-1, 4).T)


def unplanes(p, shape):
    return np.ascontiguousarray(p.T).view(np.float32).reshape(shape)


def save_npz(path, arrays):
    """An .npz as numpy writes it, with LZMA members: the mantissa planes do not pack at all, and deflate leaves the file 2 % above
    the largest ``*_parent.npz`` beside it.  ``numpy.load`` reads it like any other."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_LZMA) as z:
        for k, v in arrays.items():
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(v), allow_pickle=False)
            z.writestr(k + ".npy", b.getvalue())


def workspace_views(bufs):
    """(counts (N,) int32, keys (N, P) int64, cls (N, A) int16) views of an NmsBuffers workspace (csrc/nms_ws.h)."""
    n, A = bufs.batch, bufs.anchors
    P = 1 << (A - 1).bit_length()
    off = (4 * n + 255) // 256 * 256
    ws = bufs.workspace
    return ws[: 4 * n].view(torch.int32), ws[off : off + n * P * 8].view(torch.int64).view(n, P), ws[off + n * P * 8 : off + n * P * 8 + n * A * 2].view(torch.int16).view(n, A)


def run_case(H, kernel, nc, device):
    """Runs one case on the device: dict of the four arrays described at the top (numpy), keyed without the case name."""
    x = case_inputs(kernel, nc)
    m = class_mask(nc)
    dm = m.to(device) if m is not None else None
    bufs = H.NmsBuffers(BATCH, ANCHORS, 300, device)
    if kernel == "decode":
        # rows at pitch 76 through the descriptor itself: a view of one image of one pixel does not carry its pitch (hip_ops.view_params)
        y = torch.empty((BATCH, 4 + nc, ANCHORS), dtype=torch.float32, device=device)
        d, levels = H.DecodeDesc(), []
        for i, f in enumerate(x["feats"]):
            n, c, h, w = f.shape
            buf = torch.zeros((n, h, w, 76), dtype=torch.float32, device=device)
            buf[..., :c] = f.permute(0, 2, 3, 1).to(device)
            levels.append(buf)
            d.level[i], d.h[i], d.w[i], d.ld[i], d.stride[i] = buf.data_ptr(), h, w, 76, STRIDES[i]
        d.n_levels, d.batch, d.nc, d.reg_max, d.out = len(levels), BATCH, nc, 16, y.data_ptr()
        d.nms_workspace, d.nms_workspace_bytes, d.conf_thres = bufs.workspace.data_ptr(), bufs.workspace.numel(), CONF
        d.classes_mask = dm.data_ptr() if dm is not None else None
        H._launch(H.lib().dy_detect_decode, (ctypes.byref(d),), keep=(d, y, bufs, dm, *levels))
    else:
        dt = head_dtype(kernel, H)
        assert H.head_decode_supported(64, 64, nc, 16, dt)
        dxb = [H.to_nhwc(t.to(device), dt) for t in x["xb"]]
        dxc = [H.to_nhwc(t.to(device), dt) for t in x["xc"]]
        pb = [H.pack_frag1x1(x["wb"][i], x["bb"][i], dt, device) for i in range(len(SHAPES))]
        pc = [H.pack_frag1x1(x["wc"][i], x["bc"][i], dt, device) for i in range(len(SHAPES))]
        y = H.detect_head_decode(dxb, dxc, pb, pc, STRIDES, nc, 16, nms_bufs=bufs, conf_thres=CONF, classes_mask=dm)
    torch.cuda.synchronize()
    counts, keys, cls = (t.cpu().numpy() for t in workspace_views(bufs))
    skeys, scls = [], []
    for b in range(BATCH):
        k = np.sort(keys[b, : counts[b]].view(np.uint64))
        skeys.append(k)
        scls.append(cls[b].view(np.uint16)[(k & np.uint64(0xFFFFFFFF)).astype(np.int64)])
    return dict(pred=y.cpu().numpy(), counts=counts.copy(), keys=np.concatenate(skeys), cls=np.concatenate(scls))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "detect_rows_parent.npz"))
    a = ap.parse_args()
    from drone_yolo_amd import _lib

    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    from drone_yolo_amd import hip_ops as H

    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    arrays = {}
    for kernel, nc in CASES:
        above, kept = oracle_candidates(kernel, nc)
        r = run_case(H, kernel, nc, dev)
        print(f"{case_name(kernel, nc)}: oracle candidates {above} -> {kept} behind the mask, device {r['counts'].tolist()} of {ANCHORS}")
        assert all(0 < k < ANCHORS for k in kept) and (nc == 1 or all(k < v for k, v in zip(kept, above))), "CONF must keep some anchors and reject some"
        r["pred"] = planes(r["pred"])
        arrays.update({f"{case_name(kernel, nc)}_{k}": v for k, v in r.items()})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    save_npz(a.out, arrays)
    print(f"wrote {a.out}: {len(arrays)} arrays, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
