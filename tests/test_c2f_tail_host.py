"""CPU: dy_c2f_tail_fused's host side — the shape predicate, argument checks before any HIP call, and the descriptor's layout."""
import ctypes
import os
import subprocess
import tempfile

from tests._util import ROOT


def test_supported_predicate_truth_table():
    import drone_yolo_amd._lib as L

    f = L.lib().dy_c2f_tail_fused_supported  # (hidden, cout, n, ksize1, ksize2, groups, dtype)
    for dt in (L.DY_BF16, L.DY_F16):
        assert f(64, 128, 1, 3, 3, 1, dt) == 1 and f(64, 128, 2, 3, 3, 1, dt) == 1
        assert f(32, 128, 1, 3, 3, 1, dt) == 0 and f(128, 128, 1, 3, 3, 1, dt) == 0  # hidden
        assert f(64, 64, 1, 3, 3, 1, dt) == 0  # cout
        assert f(64, 128, 3, 3, 3, 1, dt) == 0 and f(64, 128, 0, 3, 3, 1, dt) == 0  # n
        assert f(64, 128, 1, 1, 3, 1, dt) == 0 and f(64, 128, 1, 3, 1, 1, dt) == 0  # Bottleneck kernel sizes
        assert f(64, 128, 1, 3, 3, 2, dt) == 0  # groups
    for dt in (L.DY_F32, L.DY_FP8, L.DY_F16X2):
        assert f(64, 128, 1, 3, 3, 1, dt) == 0 and f(64, 128, 2, 3, 3, 1, dt) == 0


def test_argument_checks_run_before_any_hip_call():
    import drone_yolo_amd._lib as L

    h = L.lib()
    assert h.dy_c2f_tail_fused(None, None) == -1 and b"dy_c2f_tail_fused" in h.dy_last_error_string() and b"null" in h.dy_last_error_string()
    assert h.dy_c2f_tail_fused(ctypes.byref(L.C2fTailDesc()), None) == -1 and b"null" in h.dy_last_error_string()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    d = L.C2fTailDesc()
    d.t = d.buf = d.y = d.w3 = d.b3 = d.w1 = d.b1 = p
    d.batch, d.h, d.w, d.hidden, d.cout, d.n_bottlenecks, d.ld_t, d.ld_buf, d.ld_y, d.dtype = 1, 8, 16, 32, 128, 1, 32, 64, 128, L.DY_F16
    assert h.dy_c2f_tail_fused(ctypes.byref(d), None) == -2 and b"hidden 64" in h.dy_last_error_string()  # DY_ERR_UNSUPPORTED
    d.hidden, d.ld_t, d.ld_buf = 64, 64, 64  # the buffer head holds (1 + n) * hidden channels: a pitch of 64 cannot
    assert h.dy_c2f_tail_fused(ctypes.byref(d), None) == -1 and b"pitches" in h.dy_last_error_string()
    d.ld_buf = 132  # not whole 16-byte chunks
    assert h.dy_c2f_tail_fused(ctypes.byref(d), None) == -1 and b"16-byte" in h.dy_last_error_string()


def test_descriptor_layout_matches_header():
    import drone_yolo_amd._lib as L

    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "s.c")
        open(src, "w").write('#include <stdio.h>\n#include "dyolo.h"\nint main(){printf("%zu\\n", sizeof(dy_c2f_tail_desc));return 0;}\n')
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        size = int(subprocess.check_output([exe]).split()[0])
    assert size == ctypes.sizeof(L.C2fTailDesc)
