"""Detect, Segment, OBB and Pose heads of the Drone-YOLO path (reference: ultralytics/nn/modules/head.py:21-279)."""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from ... import hip_ops as H
from .block import DFL, Proto
from .conv import Conv, DWConv, PlainConv2d
from .packs import PackOwner, packed

__all__ = ("Detect", "Segment", "OBB", "Pose")


class Detect(PackOwner, nn.Module):
    """YOLO Detect head: per level box branch cv2 and class branch cv3, then decode.

    Same constructor, attributes and state-dict keys as the reference (head.py:34-61).  Forward
    (head.py:64-74): per level the two branches write their logits into ONE fp32 NHWC buffer
    (box bins in channels [0, 4*reg_max), classes after them), which *is* ``cat(cv2(x), cv3(x), 1)``
    of the reference seen through an NHWC view.  Eval returns ``(y, x)`` with ``y`` the decoded
    (N, 4+nc, A) tensor from ``dy_detect_decode``; training mode returns the raw list ``x``.
    """

    dynamic = False
    export = False
    format = None
    end2end = False
    max_det = 300
    shape = None
    anchors = torch.empty(0)
    strides = torch.empty(0)
    legacy = False

    def __init__(self, nc=80, ch=()):
        super().__init__()
        self.nc = nc
        self.nl = len(ch)
        self.reg_max = 16
        self.no = nc + self.reg_max * 4
        self.stride = torch.zeros(self.nl)
        c2, c3 = max((16, ch[0] // 4, self.reg_max * 4)), max(ch[0], min(self.nc, 100))
        self.cv2 = nn.ModuleList(
            nn.Sequential(Conv(x, c2, 3), Conv(c2, c2, 3), PlainConv2d(c2, 4 * self.reg_max, 1)) for x in ch
        )
        self.cv3 = (
            nn.ModuleList(nn.Sequential(Conv(x, c3, 3), Conv(c3, c3, 3), PlainConv2d(c3, self.nc, 1)) for x in ch)
            if self.legacy
            else nn.ModuleList(
                nn.Sequential(
                    nn.Sequential(DWConv(x, x, 3), Conv(x, c3, 1)),
                    nn.Sequential(DWConv(c3, c3, 3), Conv(c3, c3, 1)),
                    PlainConv2d(c3, self.nc, 1),
                )
                for x in ch
            )
        )
        self.dfl = DFL(self.reg_max) if self.reg_max > 1 else nn.Identity()

    @staticmethod
    def _run_trunk(seq, x):
        """All but the last (plain 1x1) conv of one branch."""
        for m in list(seq)[:-1]:
            if isinstance(m, nn.Sequential):
                for mm in m:
                    x = mm(x)
            else:
                x = m(x)
        return x

    @classmethod
    def _run(cls, seq, x, out):
        """Run one branch; its last (plain 1x1) conv writes fp32 logits into ``out``."""
        return seq[-1](cls._run_trunk(seq, x), out=out, out_f32=True)

    fuse_tail = False  # opt-in (the predictor sets it): eval returns (y, None), the raw maps are never materialised

    def _packed_tail(self, dtype, device):
        tails = tuple(s[-1] for s in (*self.cv2, *self.cv3))

        def build():  # (in the scaled activation domain the tails divide by log2 e: the logits the decode reads are in true units)
            frags = [H.pack_frag1x1(*H.domain_fold(m.weight, m.bias, False, raw_output=True)[:2], dtype, device) for m in tails]
            return frags[: self.nl], frags[self.nl :]

        return packed(self, "tail", tails, dtype, device, build)

    def _nms_kwargs(self, n, anchors):
        """Keywords of the decode kernels' candidate filter when the predictor attached one: ``fused_nms`` = (NmsBuffers factory, conf, classes mask)."""
        fused = getattr(self, "fused_nms", None)
        if fused is None:
            return {}
        make_bufs, conf, mask = fused
        return dict(nms_bufs=make_bufs(n, anchors), conf_thres=conf, classes_mask=mask)

    fuse_first = True  # run cv2[i][0] and cv3[i][0] (same input, both 3x3) as ONE convolution on the deep levels

    def _packed_first(self, i, dtype, device):
        """cv2[i][0] and cv3[i][0] stacked along cout, or None when the level is not one the stacking pays for.

        Both read the same feature map; stacked they make a cin -> c2 + c3 3x3 layer that reads it once: from 128 input
        channels up it runs in the deep-layer GEMM kernel (conv3x3_vgemm.hip), at 64 (the P2 level, the largest map of the
        model) in the register-weight kernel (conv3x3_hreg.hip, cout 128 = two 64-cout groups that share the halo through L2).
        Same operands and fp32 accumulation per output; only the summation order over K differs from the two-launch path.
        """
        a, b = self.cv2[i][0], self.cv3[i][0]
        if not (self.fuse_first and isinstance(a, Conv) and isinstance(b, Conv) and not isinstance(a, DWConv) and not isinstance(b, DWConv)):
            return None
        ca, cb = a.conv, b.conv
        if not (ca.kernel_size == cb.kernel_size == (3, 3) and ca.stride == cb.stride == (1, 1) and ca.groups == cb.groups == 1
                and ca.in_channels == cb.in_channels and ca.in_channels >= 64 and (ca.out_channels + cb.out_channels) % 128 == 0
                and ca.out_channels % 8 == 0 and isinstance(a.act, nn.SiLU) and isinstance(b.act, nn.SiLU)):
            return None
        def build():
            (wa, ba, act), (wb, bb, _) = a._folded(), b._folded()
            return H.PackedConv(torch.cat((wa, wb), 0), torch.cat((ba, bb), 0), 1, 1, 1, act, dtype, device)

        return packed(self, ("first", i), (a, b), dtype, device, build), ca.out_channels

    def _trunks(self, i, x):
        """Outputs of the two branch trunks (all but the last 1x1 conv) of level i."""
        pf = self._packed_first(i, x.dtype, x.device)
        if pf is None:
            return self._run_trunk(self.cv2[i], x), self._run_trunk(self.cv3[i], x)
        pc, c2 = pf
        both = H.conv2d(x, pc)
        tb, tc = both[:, :c2], both[:, c2:]
        for m in list(self.cv2[i])[1:-1]:
            tb = m(tb)
        for m in list(self.cv3[i])[1:-1]:
            tc = m(tc)
        return tb, tc

    fuse_branch = True  # second 3x3 conv + 1x1 + decode of every branch in one kernel where dy_detect_branch_fused is built

    def _branches_fusable(self, dtype) -> bool:
        """Every level's branches end Conv(c, 64, 3) -> Conv(64, 64, 3) -> Conv2d(64, 4*reg_max | nc <= 16, 1) in 16-bit storage."""
        if not self.fuse_branch or self.reg_max != 16:
            return False
        for i in range(self.nl):
            for seq, kind in ((self.cv2[i], 1), (self.cv3[i], 2)):
                mods = list(seq)
                if len(mods) != 3 or not (isinstance(mods[0], Conv) and isinstance(mods[1], Conv)) or isinstance(mods[1], DWConv):
                    return False
                c1 = mods[1].conv
                if not (c1.kernel_size == (3, 3) and c1.stride == (1, 1) and c1.groups == 1 and isinstance(mods[1].act, nn.SiLU)):
                    return False
                if not H.branch_fused_supported(c1.in_channels, c1.out_channels, mods[2].out_channels, kind, self.nc, self.reg_max, dtype):
                    return False
        return True

    def _forward_branch_fused(self, x):
        """Inference with each branch's second 3x3 conv, its 1x1 conv and its share of the decode (+ NMS candidate filter) in ONE
        kernel per (level, branch): the trunk outputs never reach HBM (dy_detect_branch_fused, csrc/conv3x3_hhead.hip)."""
        n = x[0].shape[0]
        A = sum(t.shape[2] * t.shape[3] for t in x)
        dtype, dev = x[0].dtype, x[0].device
        pred = torch.empty((n, 4 + self.nc, A), dtype=torch.float32, device=dev)
        nms = self._nms_kwargs(n, A)
        if nms:
            H.nms_reset_counts(nms["nms_bufs"])
        pb, pc = self._packed_tail(dtype, dev)
        a0 = 0
        for i in range(self.nl):
            pf = self._packed_first(i, dtype, dev)
            if pf is None:
                tb, tc = self.cv2[i][0](x[i]), self.cv3[i][0](x[i])
            else:
                both = H.conv2d(x[i], pf[0])
                tb, tc = both[:, : pf[1]], both[:, pf[1] :]
            H.detect_branch_fused(tb, self.cv2[i][1]._packed_for(tb), pb[i][0], pb[i][1], 1, self.nc, self.reg_max, float(self.stride[i]), pred, a0)
            H.detect_branch_fused(tc, self.cv3[i][1]._packed_for(tc), pc[i][0], pc[i][1], 2, self.nc, self.reg_max, float(self.stride[i]), pred, a0, **nms)
            a0 += x[i].shape[2] * x[i].shape[3]
        return pred

    def _forward_fused(self, x):
        """Inference with the branch tails, decode and NMS filter in one launch (dy_detect_head_decode)."""
        if self._branches_fusable(x[0].dtype):
            return self._forward_branch_fused(x)
        tr = [self._trunks(i, x[i]) for i in range(self.nl)]
        xb, xc = [t[0] for t in tr], [t[1] for t in tr]
        pb, pc = self._packed_tail(xb[0].dtype, xb[0].device)
        kw = self._nms_kwargs(xb[0].shape[0], sum(f.shape[2] * f.shape[3] for f in xb))
        return H.detect_head_decode(xb, xc, pb, pc, [float(s) for s in self.stride], self.nc, self.reg_max, **kw)

    tail_dtype = torch.float16  # storage type of the Detect branches behind an fp8 trunk (DY_FP8 inputs): see _forward_fp8_trunk

    def _forward_fp8_trunk(self, x):
        """Levels that arrive in fp8 (BASELINE config 5: an e4m3 trunk): the FIRST 3x3 convolution of each branch reads the fp8 map on the
        block-scaled MFMA and writes ``tail_dtype`` (float16) — from there the branch is the 16-bit path: second 3x3, then the 1x1 tails +
        DFL / sigmoid decode + candidate filter in one launch where that kernel is built.  The scores and box bins, where a rounding step
        decides a detection, never pass through a 3-bit mantissa.  Inference only."""
        if self.training or not self.legacy:
            raise NotImplementedError("Detect on fp8 inputs is built for inference with the v8 (legacy) class branch")
        td = self.tail_dtype
        xb, xc = [], []
        for i in range(self.nl):
            kw = {"out_dtype": td} if x[i].dtype == H.FP8 else {}
            tb, tc = self.cv2[i][0](x[i], **kw), self.cv3[i][0](x[i], **kw)
            for m in list(self.cv2[i])[1:-1]:
                tb = m(tb)
            for m in list(self.cv3[i])[1:-1]:
                tc = m(tc)
            xb.append(tb), xc.append(tc)
        kw = self._nms_kwargs(xb[0].shape[0], sum(f.shape[2] * f.shape[3] for f in xb))
        if self.fuse_tail and H.head_decode_supported(self.cv2[0][-1].in_channels, self.cv3[0][-1].in_channels, self.nc, self.reg_max, td):
            pb, pc = self._packed_tail(td, xb[0].device)
            y = H.detect_head_decode(xb, xc, pb, pc, [float(s) for s in self.stride], self.nc, self.reg_max, **kw)
            return y if self.export else (y, None)
        nb, ld = self.reg_max * 4, (self.no + 3) // 4 * 4
        feats = []
        for i in range(self.nl):
            n, _, h, w = xb[i].shape
            buf = H.alloc_nhwc(n, self.no, h, w, torch.float32, xb[i].device, ld=ld)
            self.cv2[i][-1](xb[i], out=buf[:, :nb], out_f32=True)
            self.cv3[i][-1](xc[i], out=buf[:, nb:], out_f32=True)
            feats.append(buf)
        y = H.detect_decode(feats, [float(s) for s in self.stride], self.nc, self.reg_max, **kw)
        return y if self.export else (y, feats)

    def forward(self, x):
        if any(t.dtype == H.FP8 for t in x) and self.tail_dtype is not None:
            return self._forward_fp8_trunk(x)
        if self.fuse_tail and not self.training and H.head_decode_supported(
                self.cv2[0][-1].in_channels, self.cv3[0][-1].in_channels, self.nc, self.reg_max, x[0].dtype):
            y = self._forward_fused(x)
            return y if self.export else (y, None)
        nb = self.reg_max * 4
        ld = (self.no + 3) // 4 * 4  # keep every pixel row 16-byte aligned for the fp32 vector paths
        feats = []
        for i in range(self.nl):
            n, _, h, w = x[i].shape
            buf = H.alloc_nhwc(n, self.no, h, w, torch.float32, x[i].device, ld=ld)
            self._run(self.cv2[i], x[i], buf[:, :nb])
            self._run(self.cv3[i], x[i], buf[:, nb:])
            feats.append(buf)
        if self.training:
            return feats
        kw = self._nms_kwargs(feats[0].shape[0], sum(f.shape[2] * f.shape[3] for f in feats))
        y = H.detect_decode(feats, [float(s) for s in self.stride], self.nc, self.reg_max, **kw)
        return y if self.export else (y, feats)

    def bias_init(self):
        """box bias 1.0; cls bias log(5 / nc / (640/s)^2) — reference head.py:133-144."""
        for a, b, s in zip(self.cv2, self.cv3, self.stride):
            a[-1].bias.data[:] = 1.0
            b[-1].bias.data[: self.nc] = math.log(5 / self.nc / (640 / float(s)) ** 2)
            a[-1].invalidate_packed()
            b[-1].invalidate_packed()
        self.invalidate_packed()


class Segment(Detect):
    """YOLO Segment head — reference head.py:175-197: Detect plus ``proto`` (the mask prototypes of the first level) and, per level, the
    mask-coefficient branch ``cv4`` = Conv(x, c4, 3), Conv(c4, c4, 3), Conv2d(c4, nm, 1); same constructor and state-dict keys.

    Eval forward returns the reference's ``(cat([y, mc], 1), (feats, mc, p))``: y the decoded (N, 4 + nc, A), mc (N, nm, A), p
    (N, nm, mh, mw) fp32 in true units (an NHWC view).  On the predictor's fast path (``fuse_tail``) nothing is concatenated: the
    Detect kernels produce y and the candidate list as for a detection model and the return is ``(y, (None, levels, p))`` with ``levels``
    the per-level fp32 NHWC coefficient maps (N, nm, h_i, w_i) that ``dy_mask_gather`` reads.  The box and class branches go through
    every fusion of ``Detect`` unchanged.  Training: ``SegmentationModel.forward_train`` -> ``train_forward.segment_train`` (the maps of
    ``detect_train``, ``cv4`` through ``CoefTail``, ``proto`` through ``proto_train``); this module's own ``forward`` raises in training mode.
    """

    def __init__(self, nc=80, nm=32, npr=256, ch=()):
        super().__init__(nc, ch)
        self.nm = nm
        self.npr = npr
        self.proto = Proto(ch[0], self.npr, self.nm)
        c4 = max(ch[0] // 4, self.nm)
        self.cv4 = nn.ModuleList(nn.Sequential(Conv(x, c4, 3), Conv(c4, c4, 3), PlainConv2d(c4, self.nm, 1)) for x in ch)

    def coefficient_maps(self, x):
        """cv4 of every level: fp32 NHWC (N, nm, h_i, w_i), true units (the plain last conv leaves the scaled domain like the Detect tails)."""
        out = []
        for i in range(self.nl):
            n, _, h, w = x[i].shape
            buf = H.alloc_nhwc(n, self.nm, h, w, torch.float32, x[i].device, ld=(self.nm + 3) // 4 * 4)
            out.append(self._run(self.cv4[i], x[i], buf))
        return out

    def forward(self, x):
        if self.training:
            raise NotImplementedError("Segment.forward in training mode is not built: training goes through SegmentationModel.forward_train "
                                      "(nn/train_forward.py::segment_train), which returns (feats, coef_levels, proto)")
        if any(t.dtype == H.FP8 for t in x):
            raise NotImplementedError("Segment is built for the 16-bit, split-float16 and fp32 storage types")
        x = list(x)
        p = self.proto(x[0])
        levels = self.coefficient_maps(x)
        y, feats = Detect.forward(self, x)
        if self.fuse_tail:
            return y, (None, levels, p)
        bs = p.shape[0]
        mc = torch.cat([t.reshape(bs, self.nm, -1) for t in levels], 2)  # (layout glue of the module-level return only)
        return torch.cat([y, mc], 1), (feats, mc, p)


class OBB(Detect):
    """YOLO OBB head — reference head.py:200-227: Detect plus, per level, the angle branch ``cv4`` = Conv(x, c4, 3), Conv(c4, c4, 3),
    Conv2d(c4, ne, 1); same constructor ``(nc, ne=1, ch)`` and state-dict keys.

    The box and class branches go through every fusion of ``Detect`` unchanged and give the axis-aligned (N, 4 + nc, A) decode; ``dy_obb_decode``
    then turns each centre about its anchor point by the anchor's angle, which IS the reference's dist2rbox, and writes
    theta = (sigmoid(logit) - 0.25) * pi.  Training: ``OBBModel.forward_train`` -> ``train_forward.obb_train`` (the box and class maps of
    ``detect_train`` plus, per level, ``cv4`` through ``AngleTail``); this module's own ``forward`` raises in training mode.  Eval forward returns the reference's ``(cat([y, angle], 1), (feats, angle))``.  On the
    predictor's fast path (``fuse_tail``) nothing is concatenated: the return is ``(y, (None, theta, levels))`` with theta (N, A) and
    ``levels`` the per-level fp32 NHWC angle-logit maps.
    """

    ANGLE_COUT = 8  # a 1x1 convolution with ONE output channel: its pack is padded with zero rows to a width the 1x1 kernels serve; channel 0 is read

    def __init__(self, nc=80, ne=1, ch=()):
        super().__init__(nc, ch)
        self.ne = ne
        c4 = max(ch[0] // 4, self.ne)
        self.cv4 = nn.ModuleList(nn.Sequential(Conv(x, c4, 3), Conv(c4, c4, 3), PlainConv2d(c4, self.ne, 1)) for x in ch)

    def _packed_angle(self, i, dtype, device):
        m = self.cv4[i][-1]

        def build():  # (like the Detect tails the plain last conv leaves the scaled activation domain: the logits are in true units)
            w, b, act = H.domain_fold(m.weight, m.bias, False, raw_output=True)
            pad = self.ANGLE_COUT - w.shape[0]
            w = torch.cat((w, w.new_zeros((pad, *w.shape[1:]))), 0)
            b = torch.cat((b, b.new_zeros(pad)), 0)
            return H.PackedConv(w, b, 1, 0, 1, act, dtype, device, for_out_f32=True)

        return packed(self, ("angle", i), (m,), dtype, device, build)

    def angle_maps(self, x):
        """cv4 of every level: fp32 NHWC views (N, 1, h_i, w_i) of the raw angle logits, true units."""
        out = []
        for i in range(self.nl):
            n, _, h, w = x[i].shape
            buf = H.alloc_nhwc(n, self.ANGLE_COUT, h, w, torch.float32, x[i].device)
            t = self._run_trunk(self.cv4[i], x[i])
            H.conv2d(t, self._packed_angle(i, t.dtype, t.device), out=buf, out_f32=True)
            out.append(buf[:, :1])
        return out

    def forward(self, x):
        if self.training:
            raise NotImplementedError("OBB.forward in training mode is not built: training goes through OBBModel.forward_train (nn/train_forward.py::obb_train), "
                                      "which returns (feats, angle_levels) with the angle as its raw logit")
        if any(t.dtype == H.FP8 for t in x):
            raise NotImplementedError("OBB is built for the 16-bit, split-float16 and fp32 storage types")
        if self.ne != 1:
            raise NotImplementedError("OBB: one extra parameter per box (the angle) is what the rotated decode is built for")
        x = list(x)
        levels = self.angle_maps(x)
        y, feats = Detect.forward(self, x)
        theta = H.obb_decode(levels, [float(s) for s in self.stride], y, self.nc)
        if self.fuse_tail:
            return y, (None, theta, levels)
        angle = theta[:, None]
        return torch.cat([y, angle], 1), (feats, angle)


class Pose(Detect):
    """YOLO Pose head — reference head.py:230-279: Detect plus, per level, the keypoint branch ``cv4`` = Conv(x, c4, 3), Conv(c4, c4, 3),
    Conv2d(c4, nk, 1) with ``c4 = max(ch[0] // 4, nk)``; same constructor ``(nc, kpt_shape, ch)`` and state-dict keys.

    The box and class branches go through every fusion of ``Detect`` unchanged.  For the n, s and m scales c4 = nk = 51, which is no whole
    number of the channel groups the convolution kernels address (``H.chan_gran``: 16-byte chunks of a pixel row); the parameters keep the
    reference's shapes and the branch's PACKS are padded with zero rows, zero columns and zero bias entries to ``served_width`` -- a padded
    channel is SiLU(0) = 0 in either activation domain and meets zero weights in the next layer, so the logits are those of the unpadded
    branch.  ``keypoint_maps`` returns the per-level fp32 NHWC logit maps (N, nk, h_i, w_i) in true units, views into buffers of the
    padded width.  Eval forward returns the reference's ``(cat([y, pred_kpt], 1), (feats, kpt))`` with ``pred_kpt`` from ``dy_kpt_decode``;
    on the predictor's fast path (``fuse_tail``) nothing is concatenated: the return is ``(y, (None, levels))`` and the predictor decodes
    the kept anchors only.  Training mode raises: pose training is not built.
    """

    CH_GRAN = 16  # served_width rounds up to this: whole chunks of every storage type (fp32 4, 16-bit and split float16 8) and whole 16-row MFMA tiles

    def __init__(self, nc=80, kpt_shape=(17, 3), ch=()):
        super().__init__(nc, ch)
        self.kpt_shape = kpt_shape
        self.nk = kpt_shape[0] * kpt_shape[1]
        c4 = max(ch[0] // 4, self.nk)
        self.cv4 = nn.ModuleList(nn.Sequential(Conv(x, c4, 3), Conv(c4, c4, 3), PlainConv2d(c4, self.nk, 1)) for x in ch)

    @classmethod
    def served_width(cls, c: int, dtype) -> int:
        """The channel count a ``c``-channel activation of the keypoint branch is stored with: ``c`` where the convolution kernels take it
        as input and output (whole channel groups of ``dtype``, ``H.chan_gran``, and whole groups of 8, as ``split_supported`` asks of every
        layer), the next multiple of ``CH_GRAN`` otherwise."""
        g = max(H.chan_gran(dtype), 8)
        return c if c % g == 0 else -(-c // cls.CH_GRAN) * cls.CH_GRAN

    def _packed_kpt(self, i, dtype, device):
        """The three packs of ``cv4[i]`` at the served widths (c4 -> c4p between the convolutions, nk -> nkp on the logits)."""
        a, b, t = self.cv4[i]
        c4p, nkp = self.served_width(a.conv.out_channels, dtype), self.served_width(self.nk, dtype)

        def pad(w, bias, cout, cin):
            w = torch.nn.functional.pad(w.detach().float(), (0, 0, 0, 0, 0, cin - w.shape[1], 0, cout - w.shape[0]))
            return w, torch.nn.functional.pad(bias.detach().float(), (0, cout - bias.shape[0]))

        def build():
            (wa, ba, act_a), (wb, bb, act_b) = a._folded(), b._folded()
            wt, bt, act_t = H.domain_fold(t.weight, t.bias, False, raw_output=True)  # (the plain last conv leaves the scaled domain: true units)
            wa, ba = pad(wa, ba, c4p, wa.shape[1])
            wb, bb = pad(wb, bb, c4p, c4p)
            wt, bt = pad(wt, bt, nkp, c4p)
            return (H.PackedConv(wa, ba, 1, 1, 1, act_a, dtype, device), H.PackedConv(wb, bb, 1, 1, 1, act_b, dtype, device),
                    H.PackedConv(wt, bt, 1, 0, 1, act_t, dtype, device, for_out_f32=True))

        return packed(self, ("kpt", i), (a, b, t), dtype, device, build)

    def keypoint_maps(self, x):
        """cv4 of every level: fp32 NHWC views (N, nk, h_i, w_i) of the raw keypoint logits, true units."""
        out = []
        for i in range(self.nl):
            n, _, h, w = x[i].shape
            pa, pb, pt = self._packed_kpt(i, x[i].dtype, x[i].device)
            buf = H.alloc_nhwc(n, pt.cout, h, w, torch.float32, x[i].device)
            H.conv2d(H.conv2d(H.conv2d(x[i], pa), pb), pt, out=buf, out_f32=True)
            out.append(buf[:, : self.nk])
        return out

    def forward(self, x):
        if self.training:
            raise NotImplementedError("Pose.forward in training mode is not built: pose training (v8PoseLoss) is out of scope")
        if any(t.dtype == H.FP8 for t in x):
            raise NotImplementedError("Pose is built for the 16-bit, split-float16 and fp32 storage types")
        x = list(x)
        levels = self.keypoint_maps(x)
        y, feats = Detect.forward(self, x)
        if self.fuse_tail:
            return y, (None, levels)
        bs = y.shape[0]
        kpt = torch.cat([t.reshape(bs, self.nk, -1) for t in levels], 2)  # (layout glue of the module-level return only)
        pred_kpt = H.kpt_decode(levels, [float(s) for s in self.stride], self.kpt_shape)
        return torch.cat([y, pred_kpt], 1), (feats, kpt)
