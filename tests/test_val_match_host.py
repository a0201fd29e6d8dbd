"""CPU: ``dy_val_match`` checks its descriptor before any HIP call, and the ctypes mirror has the C struct's size."""
import ctypes
import os
import subprocess
import tempfile

from tests._util import ROOT


def test_val_match_refuses_bad_descriptors_without_gpu():
    import drone_yolo_amd._lib as L

    h = L.lib()
    assert h.dy_val_match(None, None) == -1
    assert h.dy_val_match(ctypes.byref(L.ValMatchDesc()), None) == -1  # DY_ERR_INVALID_ARG: a zeroed descriptor
    assert b"dy_val_match" in h.dy_last_error_string() and b"null" in h.dy_last_error_string()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    thr = (ctypes.c_float * 17)(*([0.5] * 17))

    def desc(**kw):
        d = L.ValMatchDesc()
        d.rows = d.counts = d.tp = p
        d.iouv, d.batch, d.max_det, d.n_labels, d.n_iouv = thr, 1, 4, 0, 10
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for n in (0, 17):
        assert h.dy_val_match(ctypes.byref(desc(n_iouv=n)), None) == -1
        assert b"n_iouv" in h.dy_last_error_string()
    for kw in (dict(rows=None), dict(counts=None), dict(tp=None)):
        assert h.dy_val_match(ctypes.byref(desc(**kw)), None) == -1 and b"null" in h.dy_last_error_string()
    for kw in (dict(batch=0), dict(batch=-3), dict(max_det=0), dict(max_det=-1), dict(max_det=4097)):
        assert h.dy_val_match(ctypes.byref(desc(**kw)), None) == -1 and b"bad dims" in h.dy_last_error_string()
    assert h.dy_val_match(ctypes.byref(desc(n_labels=-1)), None) == -1
    assert h.dy_val_match(ctypes.byref(desc(n_labels=3)), None) == -1 and b"label pointer" in h.dy_last_error_string()  # labels announced, none given


def test_val_match_desc_layout_matches_header():
    import drone_yolo_amd._lib as L

    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "s.c")
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "dyolo.h"\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(dy_val_match_desc), '
                             "offsetof(dy_val_match_desc, batch), offsetof(dy_val_match_desc, clip_w), offsetof(dy_val_match_desc, tp));return 0;}\n")
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        sizes = [int(v) for v in subprocess.check_output([exe]).split()]
    D = L.ValMatchDesc
    assert sizes == [ctypes.sizeof(D), D.batch.offset, D.clip_w.offset, D.tp.offset]


def test_device_match_is_a_checked_argument_and_on_by_default():
    """The key travels cfg/default.yaml -> trainer arguments -> DetectionValidator; the validator also takes it from Model.val's arguments."""
    import pytest

    from drone_yolo_amd.engine.trainer import get_cfg
    from drone_yolo_amd.engine.validator import DetectionValidator

    assert get_cfg()["device_match"] is True and get_cfg(dict(device_match=False))["device_match"] is False
    with pytest.raises(TypeError):
        get_cfg(dict(device_match=1))
    assert DetectionValidator().device_match is True and DetectionValidator(get_cfg()).device_match is True
    assert DetectionValidator(dict(device_match=False, unknown_key=1)).device_match is False


def test_label_preparation_on_cpu_tensors_has_the_bits_of_the_numpy_clip():
    """``DetectionValidator._labels`` (the one label preparation of the device loop and the host loop) on CPU tensors against the numpy clip
    the detection host loop used: ``xywh2xyxy * (w, h, w, h)``, then ``.clip``; boxes that stick out of the image included."""
    import numpy as np
    import torch

    from drone_yolo_amd.engine.validator import DetectionValidator, SegmentationValidator
    from drone_yolo_amd.utils import ops

    w, h = 640, 384
    g = torch.Generator().manual_seed(3)
    bb = torch.cat((torch.rand((40, 2), generator=g) * 1.2 - 0.1, torch.rand((40, 2), generator=g) * 0.6), 1)  # centres in [-0.1, 1.1]
    bb[0] = torch.tensor((0.5, 0.5, 2.0, 2.0))  # larger than the image
    lim = torch.tensor((w, h, w, h), dtype=torch.float32)
    old = (ops.xywh2xyxy(bb) * torch.tensor((w, h, w, h), dtype=torch.float32)).numpy()
    assert (old < 0).any() and (old[:, 2] > w).any() and (old[:, 3] > h).any()
    old[:, [0, 2]] = old[:, [0, 2]].clip(0, w)
    old[:, [1, 3]] = old[:, [1, 3]].clip(0, h)
    for v in (DetectionValidator(), SegmentationValidator()):
        new = v._labels(bb, w, h, lim).numpy()
        assert new.dtype == np.float32 and np.array_equal(new.view(np.uint32), old.view(np.uint32))
    assert tuple(DetectionValidator()._labels(bb[:0], w, h, lim).shape) == (0, 4)
