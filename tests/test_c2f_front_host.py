"""CPU: dy_c2f_front_fused's host side — the shape predicate, argument checks before any HIP call, the descriptor's layout, which layers
the graph planner hands to it, and the packed weights."""
import ctypes
import os
import subprocess
import tempfile

import torch

from tests._util import ROOT, load_yaml


def test_supported_predicate_truth_table():
    import drone_yolo_amd._lib as L

    f = L.lib().dy_c2f_front_fused_supported  # (cin, cmid, c_other, cout, ksize, stride, groups, act, dtype)
    for dt in (L.DY_BF16, L.DY_F16):
        for act in (L.DY_ACT_SILU, L.DY_ACT_SILU_L2E):
            assert f(64, 128, 0, 128, 3, 2, 1, act, dt) == 1 and f(64, 64, 128, 128, 3, 2, 1, act, dt) == 1  # forms A and B
        a = L.DY_ACT_SILU
        assert f(64, 128, 0, 128, 3, 2, 1, L.DY_ACT_NONE, dt) == 0  # the activation the kernel is built with
        assert f(32, 128, 0, 128, 3, 2, 1, a, dt) == 0 and f(128, 128, 0, 128, 3, 2, 1, a, dt) == 0  # cin
        assert f(64, 64, 0, 128, 3, 2, 1, a, dt) == 0 and f(64, 128, 128, 128, 3, 2, 1, a, dt) == 0 and f(64, 64, 64, 128, 3, 2, 1, a, dt) == 0  # (cmid, c_other) pairs
        assert f(64, 256, 0, 128, 3, 2, 1, a, dt) == 0
        assert f(64, 128, 0, 64, 3, 2, 1, a, dt) == 0 and f(64, 128, 0, 256, 3, 2, 1, a, dt) == 0  # cout = 2 * hidden = 128
        assert f(64, 128, 0, 128, 1, 2, 1, a, dt) == 0 and f(64, 128, 0, 128, 3, 1, 1, a, dt) == 0  # kernel size, stride
        assert f(64, 128, 0, 128, 3, 2, 2, a, dt) == 0  # groups
    for dt in (L.DY_F32, L.DY_FP8, L.DY_F16X2):
        assert f(64, 128, 0, 128, 3, 2, 1, L.DY_ACT_SILU, dt) == 0 and f(64, 64, 128, 128, 3, 2, 1, L.DY_ACT_SILU, dt) == 0


def test_argument_checks_run_before_any_hip_call():
    import drone_yolo_amd._lib as L

    h = L.lib()
    assert h.dy_c2f_front_fused(None, None) == -1 and b"dy_c2f_front_fused" in h.dy_last_error_string() and b"null" in h.dy_last_error_string()
    assert h.dy_c2f_front_fused(ctypes.byref(L.C2fFrontDesc()), None) == -1 and b"null" in h.dy_last_error_string()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    d = L.C2fFrontDesc()
    d.x = d.y = d.w3 = d.b3 = d.w1 = d.b1 = p
    d.batch, d.h, d.w, d.cin, d.cmid, d.c_other, d.cout, d.ld_x, d.ld_y, d.act, d.dtype = 1, 8, 32, 32, 128, 0, 128, 64, 128, L.DY_ACT_SILU, L.DY_F16
    assert h.dy_c2f_front_fused(ctypes.byref(d), None) == -2 and b"64 -> 128" in h.dy_last_error_string()  # DY_ERR_UNSUPPORTED
    d.cin, d.act = 64, L.DY_ACT_NONE
    assert h.dy_c2f_front_fused(ctypes.byref(d), None) == -2
    d.act, d.cmid, d.c_other = L.DY_ACT_SILU, 64, 128  # form B without its second source
    assert h.dy_c2f_front_fused(ctypes.byref(d), None) == -1 and b"other" in h.dy_last_error_string()
    d.other, d.ld_other = p, 64  # the second source holds 128 channels: a pitch of 64 cannot
    assert h.dy_c2f_front_fused(ctypes.byref(d), None) == -1 and b"pitches" in h.dy_last_error_string()
    d.ld_other = 132  # not whole 16-byte chunks
    assert h.dy_c2f_front_fused(ctypes.byref(d), None) == -1 and b"16-byte" in h.dy_last_error_string()
    d.ld_other, d.ld_y = 128, 64  # the output slice holds 128 channels
    assert h.dy_c2f_front_fused(ctypes.byref(d), None) == -1 and b"pitches" in h.dy_last_error_string()
    d.ld_y, d.batch, d.h, d.w = 128, 4096, 640, 640  # input view beyond 2 GiB
    assert h.dy_c2f_front_fused(ctypes.byref(d), None) == -2 and b"2 GiB" in h.dy_last_error_string()


def test_descriptor_layout_matches_header():
    import drone_yolo_amd._lib as L

    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "s.c")
        open(src, "w").write('#include <stdio.h>\n#include "dyolo.h"\nint main(){printf("%zu\\n", sizeof(dy_c2f_front_desc));return 0;}\n')
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        size = int(subprocess.check_output([exe]).split()[0])
    assert size == ctypes.sizeof(L.C2fFrontDesc)


def test_planner_picks_the_stride8_fronts_of_scale_s_only():
    import drone_yolo_amd as D

    none = frozenset()
    s = D.DetectionModel(load_yaml("yolov8-p2-repvgg.yaml", "s", 10), nc=10, verbose=False).eval()
    s._plan_graph()
    # C2f layer -> (producer, the producer's input, Concat or None, other Concat source or None)
    assert s._front_active(torch.float16, none) == {4: (3, 2, None, None), 21: (19, 18, 20, 15)}
    assert s._front_active(torch.bfloat16, none) == s._front_active(torch.float16, none)
    assert set(s._front) == {4, 21}  # the stride-16 / stride-32 pairs (5 -> 6, 22 -> 24, 7 -> 8, 25 -> 27) are not candidates
    assert s._front_active(torch.float32, none) == {} and s._front_active(torch.float16, frozenset({4})) == {21: (19, 18, 20, 15)}
    s.fuse_front = False
    assert s._front_active(torch.float16, none) == {}
    s.fuse_front = True
    s.model[4].fuse_block = False  # the layer-by-layer switch of the block covers its front
    assert set(s._front_active(torch.float16, none)) == {21}
    s.model[4].fuse_block = True
    s.train()
    assert s._front_active(torch.float16, none) == {}
    n = D.DetectionModel(load_yaml("yolov8-p2-repvgg.yaml", "n", 10), nc=10, verbose=False).eval()
    n._plan_graph()
    # stride 8: 32 -> 64 / 32 -> 32 convolutions, not built; its stride-16 pairs have the channel counts but are not candidates
    assert set(n._front) == {4, 21} and n._front_active(torch.float16, none) == {}
    # what the existing plan decides stays as it is (the Concat buffer is dropped per pass, not in the plan)
    assert s._place[19] == (20, 0) and s._place[15] == (20, 64)


def test_packed_weight_shapes_and_layouts():
    import drone_yolo_amd._lib as L
    from drone_yolo_amd import hip_ops as H

    g = torch.Generator().manual_seed(3)
    for cmid, c_other in ((128, 0), (64, 128)):
        w3, b3 = torch.randn(cmid, 64, 3, 3, generator=g), torch.randn(cmid, generator=g)
        w1, b1 = torch.randn(128, cmid + c_other, 1, 1, generator=g), torch.randn(128, generator=g)
        pk = H.PackedC2fFront((w3, b3), (w1, b1), L.DY_ACT_SILU, torch.float16, "cpu")
        assert (pk.cin, pk.cmid, pk.c_other, pk.cout, pk.act) == (64, cmid, c_other, 128, L.DY_ACT_SILU)
        assert pk.w3.dtype == torch.float16 and pk.w3.numel() == cmid * 64 * 9 and pk.w1.numel() == 128 * (cmid + c_other)
        assert torch.equal(pk.b3, b3) and torch.equal(pk.b1, b1)
        # DY_WLAYOUT_HALO3X3: 1 KB blocks [(cout tile * 2 + chunk) * 9 + tap][fragment 4], a lane = (part, cout row) with 8 channels
        img = pk.w3.view(cmid // 64, 2, 3, 3, 4, 4, 16, 8)
        ref = w3.to(torch.float16).view(cmid // 64, 4, 16, 2, 4, 8, 3, 3).permute(0, 3, 6, 7, 1, 4, 2, 5)
        assert torch.equal(img, ref)
        # DY_WLAYOUT_FRAG1X1: 1 KB blocks [k-group][fragment 8], the same lane order
        nkg = (cmid + c_other) // 32
        img1 = pk.w1.view(nkg, 8, 4, 16, 8)
        ref1 = w1.to(torch.float16).view(8, 16, nkg, 4, 8).permute(2, 0, 3, 1, 4)
        assert torch.equal(img1, ref1)
        # the same images the layer-by-layer path packs
        assert torch.equal(pk.w3, H.PackedConv(w3, b3, 2, 1, 1, True, torch.float16, "cpu").w)
        assert torch.equal(pk.w1, H.PackedConv(w1, b1, 1, 0, 1, True, torch.float16, "cpu").w)
