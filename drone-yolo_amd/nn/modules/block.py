"""Block-level modules of the Drone-YOLO path (reference: ultralytics/nn/modules/block.py).

``DFL`` (:58-76), ``Proto`` (:80-97), ``SPPF`` (:172-191), ``C2f`` (:227-249), ``Bottleneck`` (:337-350) and the fork's
own ``conv_bn`` / ``SEBlock`` / ``RepVGGBlock`` (:1365-1490).  chunk / cat inside C2f and SPPF are
done by construction: every producer writes its channel slice of one NHWC buffer.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ... import hip_ops as H
from .conv import Conv, _train_forward, fold_conv_bn
from .packs import PackOwner, _PackedMixin, packed

__all__ = ("DFL", "Proto", "SPPF", "C2f", "Bottleneck", "RepVGGBlock", "SEBlock", "conv_bn")


class DFL(nn.Module):
    """Integral of the distribution-focal-loss bins — reference block.py:58-76.

    Holds the frozen arange(c1) 1x1 conv for state-dict compatibility (``dfl.conv.weight``); the
    softmax-expectation itself is fused into ``dy_detect_decode``.
    """

    def __init__(self, c1=16):
        super().__init__()
        self.conv = nn.Conv2d(c1, 1, 1, bias=False).requires_grad_(False)
        self.conv.weight.data[:] = torch.arange(c1, dtype=torch.float).view(1, c1, 1, 1)
        self.c1 = c1

    def forward(self, x):
        raise RuntimeError("DFL is fused into Detect's decode kernel (dy_detect_decode); call Detect instead")


class Proto(_PackedMixin, nn.Module):
    """Mask prototypes of the segmentation models — reference block.py:80-97: cv1 3x3, ``upsample`` = ConvTranspose2d(c_, c_, 2, 2, 0,
    bias=True), cv2 3x3, cv3 1x1; same state-dict keys.

    The transposed convolution (kernel = stride = 2: every output pixel has ONE input pixel) runs as a 1x1 convolution c_ -> 4 c_ on the
    repacked weights plus ``dy_depth_to_space2_nhwc`` (``H.deconv2x2_as_conv1x1``).  ``cv3`` writes the prototypes in fp32, NHWC, in true
    units whatever the storage type and activation domain of the pass: the mask assembly (``dy_process_mask``) reads them as they are.
    """

    def __init__(self, c1, c_=256, c2=32):
        super().__init__()
        self.cv1 = Conv(c1, c_, k=3)
        self.upsample = nn.ConvTranspose2d(c_, c_, 2, 2, 0, bias=True)
        self.cv2 = Conv(c_, c_, k=3)
        self.cv3 = Conv(c_, c2)

    def _pack(self, dtype, device, cin_pad=None) -> H.PackedConv:
        """The pack of ``upsample`` (this module's only own launch besides its Conv children) as a 1x1 convolution."""
        w, b = H.deconv2x2_as_conv1x1(self.upsample.weight, self.upsample.bias)
        w, b, act = H.domain_fold(w, b, False)  # scaled input -> scaled output: the bias carries the domain's factor
        return H.PackedConv(w, b, 1, 0, 1, act, dtype, device)

    def _packed_cv3(self, x: torch.Tensor) -> H.PackedConv:
        """cv3 packed to LEAVE the scaled activation domain: weights / log2 e on the scaled input, the plain SiLU on the true
        pre-activation (SiLU is not homogeneous, so unlike the Detect tails the activation itself must run in true units)."""
        def build():
            w, b = fold_conv_bn(self.cv3.conv.weight, self.cv3.conv.bias, self.cv3.bn)
            if H.scaled_domain():
                w = w / H.LOG2E
            return H.PackedConv(w, b, 1, 0, 1, H.DY_ACT_SILU if isinstance(self.cv3.act, nn.SiLU) else H.DY_ACT_NONE, x.dtype, x.device, for_out_f32=True)

        return packed(self, "proto_out", (self.cv3,), x.dtype, x.device, build)

    def forward(self, x):
        if self.training:
            raise NotImplementedError("Proto.forward in training mode is not built: training goes through nn/train_forward.py::proto_train (SegmentationModel.forward_train)")
        t = self.cv1(x)
        t = H.conv_transpose2x2(t, self._packed_for(t))
        t = self.cv2(t)
        return H.conv2d(t, self._packed_cv3(t), out_f32=True)


class Bottleneck(nn.Module):
    """x + cv2(cv1(x)) when shortcut and c1 == c2 — reference block.py:337-350."""

    def __init__(self, c1, c2, shortcut=True, g=1, k=(3, 3), e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, k[0], 1)
        self.cv2 = Conv(c_, c2, k[1], 1, g=g)
        self.add = shortcut and c1 == c2

    def forward(self, x, out=None):
        if self.training:
            return _train_forward(self, "bottleneck_train", x, out=out)
        # the residual add rides in cv2's epilogue (after its SiLU, as in the reference expression)
        return self.cv2(self.cv1(x), out=out, residual=x if self.add else None)


class C2f(PackOwner, nn.Module):
    """CSP bottleneck with 2 convolutions, 'faster' variant — reference block.py:227-249."""

    def __init__(self, c1, c2, n=1, shortcut=False, g=1, e=0.5):
        super().__init__()
        self.c = int(c2 * e)
        self.cv1 = Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = Conv((2 + n) * self.c, c2, 1)
        self.m = nn.ModuleList(Bottleneck(self.c, self.c, shortcut, g, k=((3, 3), (3, 3)), e=1.0) for _ in range(n))

    # one-kernel execution where dy_c2f_fused is built for the shape (the stride-4 backbone and neck blocks); the last Bottleneck's 3x3 +
    # the closing 1x1 in one launch where dy_c2f_tail_fused is (the hidden-64 blocks at stride 8)
    fuse_block = True
    # Which forms of dy_c2f_tail_fused are dispatched, by (n, shortcut): what was measured below the sum of its own two launches
    # (profiles/README.md, round 7) — the forms Drone-YOLO-s has.  The kernel is built for the other two as well.
    fuse_tail_forms = ((1, False), (2, True))
    # Which forms of dy_c2f_front_fused are dispatched: "A" (a stride-2 3x3 64 -> 128 straight in front of cv1) and "B" (64 -> 64 as the
    # first source of a two-source Concat in front of it) — what was measured below the sum of its own two launches (profiles/README.md,
    # round 8).  The kernel is built and tested for both.
    fuse_front_forms = ("A", "B")

    def _packed_block(self, dtype, device):
        convs = (self.cv1, self.m[0].cv1, self.m[0].cv2, self.cv2)
        return packed(self, "block", convs, dtype, device, lambda: H.PackedC2f(
            *(c._folded()[:2] for c in convs), shortcut=self.m[0].add, dtype=dtype, device=device, act_l2e=H.scaled_domain()))

    def _packed_tail(self, dtype, device):
        convs = (self.m[-1].cv2, self.cv2)
        return packed(self, "tail", convs, dtype, device, lambda: H.PackedC2fTail(
            *(c._folded()[:2] for c in convs), n=len(self.m), shortcut=self.m[-1].add, dtype=dtype, device=device, act_l2e=H.scaled_domain()))

    @staticmethod
    def _down3x3(prod):
        """(cin, cout) of ``prod`` when it is a plain 3x3 stride-2 pad-1 SiLU convolution (Conv / RepVGGBlock without SE), else None."""
        if isinstance(prod, RepVGGBlock):
            c = prod.rbr_reparam if hasattr(prod, "rbr_reparam") else prod.rbr_dense.conv
            ok = isinstance(prod.se, nn.Identity) and prod.stride == 2 and prod.padding == 1 and prod.groups == 1
            return (c.in_channels, c.out_channels) if ok else None
        if type(prod) is Conv:
            c = prod.conv
            ok = c.kernel_size == (3, 3) and c.stride == (2, 2) and c.padding == (1, 1) and c.groups == 1 and isinstance(prod.act, nn.SiLU)
            return (c.in_channels, c.out_channels) if ok else None
        return None

    def front_fusable(self, prod, c_other, dtype) -> bool:
        """Whether ``prod`` (the layer whose output only this block's cv1 reads, with ``c_other`` channels of a second Concat source
        behind it) runs inside cv1's launch: inference, 16-bit storage, a dispatched form, a shape ``dy_c2f_front_fused`` is built for."""
        io = self._down3x3(prod)
        if io is None or self.training or prod.training or not self.fuse_block or ("B" if c_other else "A") not in self.fuse_front_forms:
            return False
        if self.cv1.conv.in_channels != io[1] + c_other or getattr(prod, "_raw_input", False):
            return False
        act = H.DY_ACT_SILU_L2E if H.scaled_domain() else H.DY_ACT_SILU  # what domain_fold hands both convolutions
        return isinstance(self.cv1.act, nn.SiLU) and H.c2f_front_fused_supported(io[0], io[1], c_other, self.cv1.conv.out_channels, dtype, act)

    def _packed_front(self, prod, dtype, device):
        def build():
            w3, b3, act = prod._folded()
            w1, b1, act1 = self.cv1._folded()
            assert act == act1
            return H.PackedC2fFront((w3, b3), (w1, b1), act, dtype, device)

        return packed(self, "front", (prod, self.cv1), dtype, device, build)

    def _cv1(self, x, out, front, kw):
        """[y0 | y1] into ``out``: cv1 on ``x``, or — ``front`` = (producer, other Concat source or None) — the producer's stride-2 3x3 on
        ``x`` and cv1 on its output (| other) in one launch."""
        if front is None:
            return self.cv1(x, out=out, **kw)
        prod, other = front
        return H.c2f_front_fused(x, self._packed_front(prod, x.dtype, x.device), other=other, out=out)

    def _tail_fusable(self, dtype):
        last = self.m[-1]
        return (len(self.m), bool(last.add)) in self.fuse_tail_forms and H.c2f_tail_fused_supported(
            self.c, self.cv2.conv.out_channels, len(self.m), dtype, last.cv1.conv.kernel_size[0], last.cv2.conv.kernel_size[0], last.cv2.conv.groups)

    def forward(self, x, out=None, front=None, **kw):
        """cv1 -> [y0 | y1]; y_{i+2} = m_i(y_{i+1}); cv2(cat(y)).  One buffer holds every y_i.

        ``kw`` (x2= / up2x=) is forwarded to cv1 so that a Concat(+Upsample) in front of this block
        can be folded into cv1's gather.  ``front`` = (producer module, other Concat source or None): ``x`` is the INPUT of the stride-2
        3x3 in front of this block, which runs inside cv1's launch (the caller asked ``front_fusable``).
        """
        if self.training:
            return _train_forward(self, "c2f_train", x, out=out, front=front, **kw)
        if kw.pop("fp8_internal", False):
            if front is not None:
                raise NotImplementedError("C2f: fp8 internals take the block's own input")
            return self._forward_fp8_internal(x, out)
        if front is not None and kw:
            raise NotImplementedError(f"C2f: front= does not combine with {sorted(kw)}")
        if self.fuse_block and len(self.m) == 1 and front is None:
            cout = self.cv2.conv.out_channels
            if not kw and H.c2f_fused_supported(x.shape[1], self.c, cout, 1, x.dtype):
                return H.c2f_fused(x, self._packed_block(x.dtype, x.device), out=out)
            x2 = kw.get("x2")
            if kw.get("up2x") and x2 is not None and len(kw) == 2 and H.c2f_fused_supported(x.shape[1] + x2.shape[1], self.c, cout, 1, x.dtype, cin_lo=x.shape[1]):
                return H.c2f_fused(x2, self._packed_block(x.dtype, x.device), out=out, x_lo=x)  # Upsample + Concat + C2f in one launch
        n, _, hb, wb = x.shape
        h, w = (2 * hb, 2 * wb) if kw.get("up2x") else (hb, wb)
        if front is not None:
            h, w = H.conv_out_hw(hb, wb, 3, 2, 1)
        c = self.c
        if self.fuse_block and len(self.m) and self._tail_fusable(x.dtype):
            # the last Bottleneck's output never reaches memory: the buffer ends with that Bottleneck's input
            nm = len(self.m)
            ybuf = H.alloc_nhwc(n, (1 + nm) * c, h, w, x.dtype, x.device)
            self._cv1(x, ybuf[:, : 2 * c], front, kw)
            for i, m in enumerate(self.m[:-1]):
                m(ybuf[:, (1 + i) * c : (2 + i) * c], out=ybuf[:, (2 + i) * c : (3 + i) * c])
            t = self.m[-1].cv1(ybuf[:, nm * c :])
            return H.c2f_tail_fused(t, ybuf, self._packed_tail(x.dtype, x.device), out=out)
        ybuf = H.alloc_nhwc(n, (2 + len(self.m)) * c, h, w, x.dtype, x.device)
        self._cv1(x, ybuf[:, : 2 * c], front, kw)
        for i, m in enumerate(self.m):
            m(ybuf[:, (1 + i) * c : (2 + i) * c], out=ybuf[:, (2 + i) * c : (3 + i) * c])
        return self.cv2(ybuf, out=out)


def _c2f_fp8_internal(self, x, out=None):
    """C2f with its internals in e4m3 (mixed plan of BASELINE config 5, nn/tasks.py::_predict_layers): cv1 reads the 16-bit input and
    writes fp8 ([y0 | y1] in ONE fp8 buffer), every Bottleneck convolution runs fp8 -> fp8 on the block-scaled MFMA, cv2 reads the
    fp8 buffer and writes the 16-bit output — the block's boundary types are its caller's (csrc/conv_gemm_fk.hip, y_dtype1)."""
    n, _, h, w = x.shape
    c = self.c
    ybuf = H.alloc_nhwc(n, (2 + len(self.m)) * c, h, w, H.FP8, x.device)
    self.cv1(x, out=ybuf[:, : 2 * c], out_dtype=H.FP8)
    for i, m in enumerate(self.m):
        m(ybuf[:, (1 + i) * c : (2 + i) * c], out=ybuf[:, (2 + i) * c : (3 + i) * c])
    return self.cv2(ybuf, out=out, out_dtype=x.dtype)


C2f._forward_fp8_internal = _c2f_fp8_internal


class SPPF(nn.Module):
    """Spatial pyramid pooling (fast): cv1, three chained k x k max pools, cv2 — reference block.py:172-191."""

    def __init__(self, c1, c2, k=5):
        super().__init__()
        c_ = c1 // 2
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_ * 4, c2, 1, 1)
        self.k = k
        self.m = nn.MaxPool2d(kernel_size=k, stride=1, padding=k // 2)  # kept for repr / state parity only

    def forward(self, x, out=None):
        if self.training:
            return _train_forward(self, "sppf_train", x, out=out)
        n, _, h, w = x.shape
        c_ = self.cv1.conv.out_channels
        ybuf = H.alloc_nhwc(n, 4 * c_, h, w, x.dtype, x.device)
        self.cv1(x, out=ybuf[:, :c_])
        H.sppf_maxpool3(ybuf[:, :c_], ybuf[:, c_ : 2 * c_], ybuf[:, 2 * c_ : 3 * c_], ybuf[:, 3 * c_ :], self.k)
        return self.cv2(ybuf, out=out)


def conv_bn(in_channels, out_channels, kernel_size, stride, padding, groups=1):
    """Sequential(conv(bias=False), bn) with the reference's child names — block.py:1365-1372."""
    result = nn.Sequential()
    result.add_module("conv", nn.Conv2d(in_channels, out_channels, kernel_size, stride, padding, groups=groups, bias=False))
    result.add_module("bn", nn.BatchNorm2d(out_channels))
    return result


class SEBlock(nn.Module):
    """Squeeze-excite gate of RepVGGBlock(use_se=True) — reference block.py:1374-1391.

    Parameter container only: no Drone-YOLO YAML enables it (use_se defaults to False), so no
    kernel is built for it and ``forward`` refuses rather than falling back to eager PyTorch.
    """

    def __init__(self, input_channels, internal_neurons):
        super().__init__()
        self.down = nn.Conv2d(input_channels, internal_neurons, kernel_size=1, stride=1, bias=True)
        self.up = nn.Conv2d(internal_neurons, input_channels, kernel_size=1, stride=1, bias=True)
        self.input_channels = input_channels

    def forward(self, inputs):
        raise NotImplementedError("SEBlock (RepVGGBlock use_se=True) has no HIP kernel: not on the Drone-YOLO path")


class RepVGGBlock(_PackedMixin, nn.Module):
    """RepVGG block: SiLU(BN(conv3x3) + BN(conv1x1) + BN(identity)) — reference block.py:1393-1490.

    The three branches are folded into ONE 3x3 kernel and bias when the weights are packed
    (``get_equivalent_kernel_bias``, :1446-1478), so the device always runs the deploy form; the
    state dict keeps the training-time keys (``rbr_dense.conv.weight``, ``rbr_1x1.bn.*`` ...).
    """

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1, dilation=1, groups=1,
                 padding_mode="zeros", deploy=False, use_se=False):
        super().__init__()
        if dilation != 1 or padding_mode != "zeros" or kernel_size != 3:
            raise NotImplementedError("RepVGGBlock is built for 3x3, dilation 1, zero padding")
        self.deploy = deploy
        self.groups = groups
        self.in_channels = in_channels
        self.stride, self.padding = stride, padding
        padding_11 = padding - kernel_size // 2
        self.nonlinearity = nn.SiLU()
        self.se = SEBlock(out_channels, internal_neurons=out_channels // 16) if use_se else nn.Identity()
        if deploy:
            self.rbr_reparam = nn.Conv2d(in_channels, out_channels, kernel_size, stride, padding, dilation=dilation,
                                         groups=groups, bias=True, padding_mode=padding_mode)
        else:
            self.rbr_identity = nn.BatchNorm2d(in_channels) if out_channels == in_channels and stride == 1 else None
            self.rbr_dense = conv_bn(in_channels, out_channels, kernel_size, stride, padding, groups=groups)
            self.rbr_1x1 = conv_bn(in_channels, out_channels, 1, stride, padding_11, groups=groups)

    # -- folding (reference block.py:1446-1478) ---------------------------------------------------
    def _fuse_bn_tensor(self, branch):
        if branch is None:
            return 0, 0
        if isinstance(branch, nn.Sequential):
            return fold_conv_bn(branch.conv.weight, None, branch.bn)
        input_dim = self.in_channels // self.groups  # identity branch: a 3x3 kernel with a centre 1
        k = torch.zeros((self.in_channels, input_dim, 3, 3), dtype=torch.float32, device=branch.weight.device)
        k[torch.arange(self.in_channels), torch.arange(self.in_channels) % input_dim, 1, 1] = 1.0
        return fold_conv_bn(k, None, branch)

    def get_equivalent_kernel_bias(self):
        k3, b3 = self._fuse_bn_tensor(self.rbr_dense)
        k1, b1 = self._fuse_bn_tensor(self.rbr_1x1)
        kid, bid = self._fuse_bn_tensor(getattr(self, "rbr_identity", None))
        k1 = torch.nn.functional.pad(k1, [1, 1, 1, 1]) if isinstance(k1, torch.Tensor) else 0
        return k3 + k1 + kid, b3 + b1 + bid

    def switch_to_deploy(self):
        """Replace the branches by the folded conv, as the reference's switch_to_deploy (:1421-1444)."""
        if hasattr(self, "rbr_1x1"):
            kernel, bias = self.get_equivalent_kernel_bias()
            d = self.rbr_dense.conv
            self.rbr_reparam = nn.Conv2d(d.in_channels, d.out_channels, d.kernel_size, d.stride, d.padding,
                                         dilation=d.dilation, groups=d.groups, bias=True)
            self.rbr_reparam.weight.data = kernel.to(d.weight.device)
            self.rbr_reparam.bias.data = bias.to(d.weight.device)
            for p in self.parameters():
                p.detach_()
            del self.rbr_dense, self.rbr_1x1
            if hasattr(self, "rbr_identity"):
                del self.rbr_identity
            self.deploy = True
            self.invalidate_packed()

    def _folded(self):
        """(weight, bias, activation code) of the deploy form, for the activation domain in force (``H.domain_fold``)."""
        if hasattr(self, "rbr_reparam"):
            w, b = self.rbr_reparam.weight, self.rbr_reparam.bias
        else:
            w, b = self.get_equivalent_kernel_bias()
        return H.domain_fold(w, b, True, raw_input=getattr(self, "_raw_input", False))

    def _pack(self, dtype, device, cin_pad=None) -> H.PackedConv:
        w, b, act = self._folded()
        return H.PackedConv(w, b, self.stride, self.padding, self.groups, act, dtype, device, cin_pad=cin_pad)

    def forward(self, inputs, out=None):
        if not isinstance(self.se, nn.Identity):
            return self.se(inputs)  # raises: no SE kernel
        if self.training:
            return _train_forward(self, "repvgg_train", inputs, out=out)
        return H.conv2d(inputs, self._packed_for(inputs), out=out)
