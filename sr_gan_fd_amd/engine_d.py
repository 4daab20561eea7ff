"""HIP engine for the U-Net discriminator (spectral-normalised).

Reference: DiscriminatorUNet._forward_impl BSRGAN/model.py:141-167 with torch's spectral_norm
(torch/nn/utils/spectral_norm.py:62-114) applied at :104-132.

Discriminator data flow (NHWC, one buffer per saved activation):
  x(3->32 pad) -conv1-> out1 -4x4s2-> d1 -4x4s2-> d2 -4x4s2-> d3 -bilinear-> b3 -conv-> (+d2) u1
  -bilinear-> b2 -conv-> (+d1) u2 -bilinear-> b1 -conv-> (+out1) u3 -conv-> c2 -conv-> c3 -conv4-> logits(fp32)
Spectral norm: per training forward one power iteration (HIP kernels) updates weight_u / weight_v in
place and produces 1/sigma on the device; the weight packer multiplies it in, so the conv kernels see
W/sigma without an extra pass.  Backward: dL/d(W/sigma) from the wgrad kernel goes through
srganfd_spectral_norm_grad (both the 1/sigma path and the -<G,W>/sigma^2 u v^T path).
The stride-2 data gradient runs as 4 output-parity classes, each a 2x2-tap stride-1 conv.
The spectral-norm plumbing is engine_core.py's; the passes over the launch lists and the autograd glue are engine.py's (EngineBase).
"""
from __future__ import annotations

import torch
from torch import Tensor, nn

from . import _abi as A
from . import ops
from .engine import _engine, _Shape, engine_apply
from .engine_core import DiscriminatorEngineCore, first_layer_dgrad

SN_LAYERS = [("down_block1", 4, 2), ("down_block2", 4, 2), ("down_block3", 4, 2), ("up_block1", 3, 1),
             ("up_block2", 3, 1), ("up_block3", 3, 1), ("conv2", 3, 1), ("conv3", 3, 1)]


class DiscriminatorEngine(DiscriminatorEngineCore):
    what = "DiscriminatorUNet"

    def __init__(self, owner: nn.Module):
        super().__init__(owner, owner.conv1.weight.shape[1], [f"{n}.0.weight_orig" for n, _, _ in SN_LAYERS])
        self.out_ch = owner.conv4.weight.shape[0]
        if owner.down_block1[0].weight_orig.shape[1] != 64 or owner.conv1.weight.shape[0] != 64:
            raise A.SrganfdError("DiscriminatorUNet: conv1 hard-codes 64 outputs (model.py:102), so channels must be 64")
        if self.out_ch != 1:
            raise A.SrganfdError("DiscriminatorUNet out_channels must be 1 (logits are written NCHW == NHWC)")

    # ---- packing: every operand carries 1/sigma of its layer (scalars[2*l+1]) ----
    def _build_pack(self, dtc: int, device) -> dict:
        pb = ops.PackBuilder(dtc)
        for name, co, ci in (("conv1", 64, self.in_ch), ("conv4", self.out_ch, 64)):
            pb.fwd(("f", name), self._poff(name + ".weight"), co, ci)
            pb.bwd(("b", name), self._poff(name + ".weight"), co, ci)
        for l, (name, k, s) in enumerate(SN_LAYERS):
            pname, co, cols = self.sn[l]
            src, ci = self._poff(pname), cols // (k * k)
            pb.fwd(("f", name), src, co, ci, k, scale_off=2 * l + 1)
            if s == 1:
                pb.bwd(("b", name), src, co, ci, k, scale_off=2 * l + 1)
            else:
                pb.classes(("b", name), src, co, ci, 2, 2, scale_off=2 * l + 1)
        return pb.finish(device)

    # ---- per-shape plan ----
    def _plan_forward(self, sp: _Shape, b: ops.PlanBuilder, train: bool) -> None:
        H, W = sp.H, sp.W
        if H % 8 or W % 8:
            raise A.SrganfdError("DiscriminatorUNet input height/width must be multiples of 8")
        # conv1 (in_ch -> 64) and conv4 (64 -> out_ch) on the thin-side kernels in the 16-bit modes (csrc/conv_thin.hip): 4-channel pitch
        sp.thin_i, sp.thin_o = ops.thin_ok(sp.dtc, 64, self.in_ch), ops.thin_ok(sp.dtc, 64, self.out_ch)
        sp.xin = b.act(H, W, 4 if sp.thin_i else 32)
        sp.out1 = b.act(H, W, 64)
        sp.d1, sp.d2, sp.d3 = b.act(H // 2, W // 2, 128), b.act(H // 4, W // 4, 256), b.act(H // 8, W // 8, 512)
        sp.b3, sp.u1 = b.act(H // 4, W // 4, 512), b.act(H // 4, W // 4, 256)
        sp.b2, sp.u2 = b.act(H // 2, W // 2, 256), b.act(H // 2, W // 2, 128)
        sp.b1, sp.u3 = b.act(H, W, 128), b.act(H, W, 64)
        sp.c2, sp.c3 = b.act(H, W, 64), b.act(H, W, 64)
        # LeakyReLU outputs before the skip adds (exact derivative sign in backward)
        sp.a1, sp.a2, sp.a3 = b.act(H // 4, W // 4, 256), b.act(H // 2, W // 2, 128), b.act(H, W, 64)
        V = A.view
        lre = dict(act=A.ACT_LRELU, slope=0.2)
        sp.fw = [
            b.image_to_features(sp.thin_i, sp.xin, sp.out1, "conv1", H, W, self.in_ch, 64, True),
            b.conv(sp.out1, sp.d1, ("f", "down_block1"), H, W, 64, 128, ksize=4, stride=2, **lre),
            b.conv(sp.d1, sp.d2, ("f", "down_block2"), H // 2, W // 2, 128, 256, ksize=4, stride=2, **lre),
            b.conv(sp.d2, sp.d3, ("f", "down_block3"), H // 4, W // 4, 256, 512, ksize=4, stride=2, **lre),
            b.resample(1, sp.d3, sp.b3, H // 8, W // 8, 512),
            b.conv(sp.b3, sp.u1, ("f", "up_block1"), H // 4, W // 4, 512, 256, r1=V(sp.d2), r1_scale=1.0, y2=V(sp.a1), **lre),
            b.resample(1, sp.u1, sp.b2, H // 4, W // 4, 256),
            b.conv(sp.b2, sp.u2, ("f", "up_block2"), H // 2, W // 2, 256, 128, r1=V(sp.d1), r1_scale=1.0, y2=V(sp.a2), **lre),
            b.resample(1, sp.u2, sp.b1, H // 2, W // 2, 128),
            b.conv(sp.b1, sp.u3, ("f", "up_block3"), H, W, 128, 64, r1=V(sp.out1), r1_scale=1.0, y2=V(sp.a3), **lre),
            b.conv(sp.u3, sp.c2, ("f", "conv2"), H, W, 64, 64, **lre),
            b.conv(sp.c2, sp.c3, ("f", "conv3"), H, W, 64, 64, **lre),
            # conv4 writes the logits, allocated per forward
            ops.PerCall(b.features_to_image(sp.thin_o, sp.c3, 0, 1, "conv4", H, W, 1, 64, False)),
        ]

    def _plan_backward(self, sp: _Shape, b: ops.PlanBuilder) -> None:
        H, W = sp.H, sp.W
        sp.dl = b.act(H, W, 4 if sp.thin_o else 32)
        sp.thin_ws = b.thin_ws(sp.thin_i, sp.thin_o)
        gA, gB, gC, gD = b.act(H, W, 64), b.act(H, W, 64), b.act(H, W, 128), b.act(H, W, 64)
        h1, h2, h3, h4 = b.act(H // 2, W // 2, 128), b.act(H // 2, W // 2, 128), b.act(H // 2, W // 2, 256), b.act(H // 2, W // 2, 128)
        q1, q2, q3, q4 = b.act(H // 4, W // 4, 256), b.act(H // 4, W // 4, 256), b.act(H // 4, W // 4, 512), b.act(H // 4, W // 4, 256)
        e1 = b.act(H // 8, W // 8, 512)
        sp.dxp = b.act(H, W, 4, dtype=torch.float32)
        sp.keep = [gA, gB, gC, gD, h1, h2, h3, h4, q1, q2, q3, q4, e1]

        def sn_wgrad(l, x, dy, h, w, cin, cout, **kw):
            """weight gradient of spectral-normalised layer l: dL/d(W/sigma) goes to the scratch gradient, SnGradBatch finishes the job"""
            return b.wgrad(x, dy, h, w, cin, cout, self.sn[l][0], sn=l, **kw)
        down = dict(ksize=4, stride=2, pad=1)
        bw = [
            b.image_wgrad(sp.thin_o, sp.dl, sp.c3, "conv4", sp.thin_ws, H, W, 1, 64, False),
            b.image_to_features(sp.thin_o, sp.dl, gA, "conv4", H, W, 1, 64, False, flip=True, mask=A.view(sp.c3), mask_slope=0.2),
            sn_wgrad(7, sp.c2, gA, H, W, 64, 64),
            b.dgrad(gA, gB, ("b", "conv3"), H, W, 64, 64, mask=sp.c2),
            sn_wgrad(6, sp.u3, gB, H, W, 64, 64),
            # u3 = lrelu(z3) + out1: the conv's two outputs are d u3 (y2: the skip's share, added into d out1 below) and
            # d z3 = d u3 * lrelu'(a3) (y, after the mask) -- no separate LeakyReLU-backward pass over the 512^2 tensor
            b.dgrad(gB, gD, ("b", "conv2"), H, W, 64, 64, mask=sp.a3, y2=A.view(gA)),              # gA = d u3, gD = d z3
            sn_wgrad(5, sp.b1, gD, H, W, 128, 64),
            b.dgrad(gD, gC, ("b", "up_block3"), H, W, 64, 128),                                  # gC = d b1
            b.resample_bwd_lrelu(gC, h1, sp.a2, h2, H // 2, W // 2, 128),                        # h1 = d u2, h2 = d z2
            sn_wgrad(4, sp.b2, h2, H // 2, W // 2, 256, 128),
            b.dgrad(h2, h3, ("b", "up_block2"), H // 2, W // 2, 128, 256),                       # h3 = d b2
            b.resample_bwd_lrelu(h3, q1, sp.a1, q2, H // 4, W // 4, 256),                        # q1 = d u1, q2 = d z1
            sn_wgrad(3, sp.b3, q2, H // 4, W // 4, 512, 256),
            b.dgrad(q2, q3, ("b", "up_block1"), H // 4, W // 4, 256, 512),                       # q3 = d b3
            b.resample_bwd_lrelu(q3, A.NULL_VIEW, sp.d3, e1, H // 8, W // 8, 512),               # e1 = d d3 (pre-activation)
            sn_wgrad(2, sp.d2, e1, H // 4, W // 4, 256, 512, **down),
        ]
        # the 4x4 stride-2 data gradients: 4 output-parity classes (2x2-tap convs over dy)
        bw += b.strided_dgrad(e1, q4, ("b", "down_block3"), H // 8, W // 8, 512, 256, 2, 1, r1=q1, mask=sp.d2)     # q4 = (d d2 + d u1) * lrelu'(d2)
        bw.append(sn_wgrad(1, sp.d1, q4, H // 2, W // 2, 128, 256, **down))
        bw += b.strided_dgrad(q4, h4, ("b", "down_block2"), H // 4, W // 4, 256, 128, 2, 1, r1=h1, mask=sp.d1)     # h4 = (d d1 + d u2) * lrelu'(d1)
        bw.append(sn_wgrad(0, sp.out1, h4, H, W, 64, 128, **down))
        bw += b.strided_dgrad(h4, gD, ("b", "down_block1"), H // 2, W // 2, 128, 64, 2, 1, r1=gA)                  # gD = d out1 (+ skip d u3)
        bw.append(b.image_wgrad(sp.thin_i, sp.xin, gD, "conv1", sp.thin_ws, H, W, self.in_ch, 64, True))
        sp.dx_conv = first_layer_dgrad(b.features_to_image(sp.thin_i, gD, sp.dxp, 4, "conv1", H, W, self.in_ch, 64, True, flip=True))
        sp.bw = bw
        self._backward_workspaces(sp, b)


def discriminator_engine(owner: nn.Module) -> DiscriminatorEngine:
    return _engine(owner, lambda: DiscriminatorEngine(owner))


def discriminator_apply(owner: nn.Module, x: Tensor) -> Tensor:
    return engine_apply(discriminator_engine(owner), x, owner.training)
