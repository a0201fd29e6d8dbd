"""Inputs of the pose fixtures, shared by tools/make_pose_golden.py and the tests (not collected).  Everything is regenerated from a seed
(torch.Generator on the CPU); tests/golden/pose.npz stores the seeds and what the reference returned."""
import numpy as np
import torch

HEADS = {"a": dict(nc=1, kpt_shape=(17, 3)), "b": dict(nc=3, kpt_shape=(4, 2))}  # the two head vectors: Pose(nc, kpt_shape, ch=(32, 64))
HEAD_CH, HEAD_MAPS = (32, 64), ((2, 32, 8, 12), (2, 64, 4, 6))
HEAD_STRIDES = (8.0, 16.0)

DECODE_BATCH = 2
DECODE_LEVELS = ((5, 7, 8.0), (3, 4, 16.0))  # (h, w, stride): odd sizes, two levels
DECODE_SHAPES = {"dec3": (17, 3), "dec2": (4, 2)}


def randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def decode_logits(seed, kpt_shape):
    """Per level the (B, nk, h, w) keypoint logits: N(0, 3), with saturated visibilities at the first and last anchor of every level."""
    nk = kpt_shape[0] * kpt_shape[1]
    out = []
    for i, (h, w, _) in enumerate(DECODE_LEVELS):
        t = randn(seed + i, DECODE_BATCH, nk, h, w) * 3.0
        if kpt_shape[1] == 3:
            t[0, 2::3, 0, 0], t[1, 2::3, 0, 0] = -40.0, 40.0
            t[0, 2::3, h - 1, w - 1], t[1, 2::3, h - 1, w - 1] = 90.0, -90.0
        out.append(t)
    return out


def padded_levels(logits, device, extra=5, poison=1e30):
    """The logits as fp32 NHWC views (B, nk, h, w) with a pixel pitch of nk + extra, the rest of every pixel row poison."""
    views = []
    for t in logits:
        b, nk, h, w = t.shape
        buf = torch.full((b, h, w, nk + extra), poison, dtype=torch.float32, device=device)
        buf[..., :nk] = t.permute(0, 2, 3, 1).to(device)
        views.append(buf.permute(0, 3, 1, 2)[:, :nk])
    return views


# scale_coords cases: name -> (input hw, original hw); one has a non-integer pad on x, the other on y
SCALE_CASES = {"pad_x": ((96, 128), (90, 100)), "pad_y": ((96, 128), (75, 113))}


def scale_inputs(seed, in_hw, n=6, nkpt=17):
    """(n, nkpt, 3) keypoints in input pixels: some beyond every image edge, visibilities on both sides of 0.5 (none within 0.01 of it)."""
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(n, nkpt, 2, generator=g) * torch.tensor([in_hw[1] + 40.0, in_hw[0] + 40.0]) - 20.0
    v = torch.rand(n, nkpt, 1, generator=g)
    v = torch.where((v - 0.5).abs() < 0.01, v + 0.05, v)
    return torch.cat((xy, v), 2).contiguous()


# the five crops of the (2, 90, 140) frame pair (frame, xyxy box) at crop_expand = 0.2 and imgsz = 64: cut at the top-left corner, cut at
# the bottom-right corner, exactly imgsz wide after the expansion, tall, and 9 x 7 (upscaled)
CROP_FRAMES_HW = (90, 140)
CROP_EXPAND = 0.2
CROP_BOXES = [np.array([[2.0, 3.0, 40.0, 33.0], [100.0, 60.0, 138.0, 88.0], [30.0, 20.0, 75.5, 50.0]]),
              np.array([[60.0, 5.0, 75.0, 80.0], [50.0, 40.0, 56.5, 45.0]])]
CROP_RECTS = [(0, 0, 0, 47, 39), (0, 92, 54, 140, 90), (0, 20, 14, 84, 56), (1, 57, 0, 78, 90), (1, 48, 39, 57, 46)]  # (frame, x0, y0, x1e, y1e): worked by hand


def crop_frames(seed=11):
    return np.random.default_rng(seed).integers(0, 256, (2, *CROP_FRAMES_HW, 3), dtype=np.uint8)
