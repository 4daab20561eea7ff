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
    def _plan(self, N, S1, S2, dt, dtc, device, pk, train=True) -> _Shape:
        key = (N, S1, S2, dtc, str(device), pk["buf"].data_ptr(), self.fp.flat.data_ptr())
        sp = self.shapes.get(key)
        if sp is not None:
            return sp
        if S1 % 8 or S2 % 8:
            raise A.SrganfdError("DiscriminatorUNet input height/width must be multiples of 8")
        sp = _Shape()
        sp.N, sp.H, sp.W, sp.dt, sp.dtc, sp.device = N, S1, S2, dt, dtc, device
        V = A.view
        fptr, wptr = self.fp.flat.data_ptr(), pk["buf"].data_ptr()
        O = pk["offs"]

        def new(h, w, c, dtype=dt):
            return torch.empty(N, h, w, c, dtype=dtype, device=device)
        H, W = S1, S2
        # conv1 (in_ch -> 64) and conv4 (64 -> out_ch) on the thin-side kernels in the 16-bit modes (csrc/conv_thin.hip): 4-channel pitch
        sp.thin_i, sp.thin_o = ops.thin_ok(dtc, 64, self.in_ch), ops.thin_ok(dtc, 64, self.out_ch)
        sp.xin = new(H, W, 4 if sp.thin_i else 32)
        sp.out1 = new(H, W, 64)
        sp.d1, sp.d2, sp.d3 = new(H // 2, W // 2, 128), new(H // 4, W // 4, 256), new(H // 8, W // 8, 512)
        sp.b3, sp.u1 = new(H // 4, W // 4, 512), new(H // 4, W // 4, 256)
        sp.b2, sp.u2 = new(H // 2, W // 2, 256), new(H // 2, W // 2, 128)
        sp.b1, sp.u3 = new(H, W, 128), new(H, W, 64)
        sp.c2, sp.c3 = new(H, W, 64), new(H, W, 64)
        # LeakyReLU outputs before the skip adds (exact derivative sign in backward)
        sp.a1, sp.a2, sp.a3 = new(H // 4, W // 4, 256), new(H // 2, W // 2, 128), new(H, W, 64)
        cv = lambda *a, **k: ops.Conv(ops.conv_args(dtc, *a, **k))
        rs = lambda op, a, b, h, w, c: ops.Call("srganfd_resample", (op, a, b, dtc, N, h, w, c), "resample")
        lre = dict(act=A.ACT_LRELU, slope=0.2)
        w1, b1 = fptr + 4 * self._poff("conv1.weight"), fptr + 4 * self._poff("conv1.bias")
        fw = [
            ops.image_to_features(dtc, sp.thin_i, sp.xin, V(sp.out1), w1, wptr + O[("f", "conv1")], N, H, W, self.in_ch, 64, True, bias=b1),
            cv(V(sp.out1), V(sp.d1), wptr + O[("f", "down_block1")], N, H, W, 64, 128, ksize=4, stride=2, **lre),
            cv(V(sp.d1), V(sp.d2), wptr + O[("f", "down_block2")], N, H // 2, W // 2, 128, 256, ksize=4, stride=2, **lre),
            cv(V(sp.d2), V(sp.d3), wptr + O[("f", "down_block3")], N, H // 4, W // 4, 256, 512, ksize=4, stride=2, **lre),
            rs(1, V(sp.d3), V(sp.b3), H // 8, W // 8, 512),
            cv(V(sp.b3), V(sp.u1), wptr + O[("f", "up_block1")], N, H // 4, W // 4, 512, 256, r1=V(sp.d2), r1_scale=1.0, y2=V(sp.a1), **lre),
            rs(1, V(sp.u1), V(sp.b2), H // 4, W // 4, 256),
            cv(V(sp.b2), V(sp.u2), wptr + O[("f", "up_block2")], N, H // 2, W // 2, 256, 128, r1=V(sp.d1), r1_scale=1.0, y2=V(sp.a2), **lre),
            rs(1, V(sp.u2), V(sp.b1), H // 2, W // 2, 128),
            cv(V(sp.b1), V(sp.u3), wptr + O[("f", "up_block3")], N, H, W, 128, 64, r1=V(sp.out1), r1_scale=1.0, y2=V(sp.a3), **lre),
            cv(V(sp.u3), V(sp.c2), wptr + O[("f", "conv2")], N, H, W, 64, 64, **lre),
            cv(V(sp.c2), V(sp.c3), wptr + O[("f", "conv3")], N, H, W, 64, 64, **lre),
        ]
        # conv4 writes the logits, allocated per forward
        fw.append(ops.PerCall(ops.features_to_image(dtc, sp.thin_o, V(sp.c3), 0, 1, fptr + 4 * self._poff("conv4.weight"), wptr + O[("f", "conv4")],
                                                    N, H, W, 1, 64, False, bias=fptr + 4 * self._poff("conv4.bias"))))
        sp.fw = fw
        self._plan_backward(sp, pk)
        self.shapes[key] = sp
        return sp

    def _plan_backward(self, sp: _Shape, pk: dict) -> None:
        N, H, W, dt, dtc, device = sp.N, sp.H, sp.W, sp.dt, sp.dtc, sp.device
        V = A.view
        wptr, O = pk["buf"].data_ptr(), pk["offs"]

        def new(h, w, c, dtype=dt):
            return torch.empty(N, h, w, c, dtype=dtype, device=device)
        sp.dl = new(H, W, 4 if sp.thin_o else 32)
        fptr = self.fp.flat.data_ptr()
        sp.thin_ws = torch.empty(ops.thin_wgrad_workspace_bytes(), dtype=torch.uint8, device=device) if (sp.thin_i or sp.thin_o) else None
        gA, gB, gC, gD = new(H, W, 64), new(H, W, 64), new(H, W, 128), new(H, W, 64)
        h1, h2, h3, h4 = new(H // 2, W // 2, 128), new(H // 2, W // 2, 128), new(H // 2, W // 2, 256), new(H // 2, W // 2, 128)
        q1, q2, q3, q4 = new(H // 4, W // 4, 256), new(H // 4, W // 4, 256), new(H // 4, W // 4, 512), new(H // 4, W // 4, 256)
        e1 = new(H // 8, W // 8, 512)
        sp.dxp = new(H, W, 4, dtype=torch.float32)
        sp.keep = [gA, gB, gC, gD, h1, h2, h3, h4, q1, q2, q3, q4, e1]
        wplans = ops.WgradPlans(device, dtc, N)

        def wg(name, x, dy, h, w, cin, cout, sn_index=None, k=3, s=1, cin_real=None, cout_real=None, bias=False):
            """weight gradient: plain params write straight into the flat gradient; SN layers write
            dL/d(W/sigma) into the temp buffer and srganfd_spectral_norm_grad finishes the job."""
            pname = self.sn[sn_index][0] if sn_index is not None else f"{name}.weight"
            plan = wplans.conv(h, w, cin, cout, self._poff(pname), self._poff(f"{name}.bias") if bias else -1, cin_real, cout_real,
                               ksize=k, stride=s, pad=1)
            return ops.Wgrad(plan, V(x), V(dy), sn=sn_index)

        cv = lambda *a, **k: ops.Conv(ops.conv_args(dtc, *a, **k))
        # bilinear-x2 backward + LeakyReLU' of the upsampled layer in one pass: raw gradient (the skip connection's share) and masked one
        rsl = lambda dy, raw, act, masked, h, w, c: ops.Call("srganfd_resample_bwd_lrelu", (dy, raw, act, masked, dtc, N, h, w, c, 0.2), "resample_bwd_lrelu")

        def s2_dgrad(name, dy, dx, hd, wd, cout, cin, r1, mask):
            """data gradient of a 4x4 stride-2 conv: 4 output-parity classes (2x2-tap convs over dy)"""
            return ops.parity_class_launches(
                dtc, V(dy), V(dx), wptr, [O[("b", name, c)] for c in range(4)], N, hd, wd, cout, cin, 2, 1,
                **ops.dgrad_epilogue(r1=None if r1 is None else V(r1), mask=None if mask is None else V(mask)))

        w4raw, w1raw = fptr + 4 * self._poff("conv4.weight"), fptr + 4 * self._poff("conv1.weight")
        bw = [
            ops.image_wgrad(dtc, sp.thin_o, wplans, sp.dl, sp.c3, w4raw, self._poff("conv4.weight"), self._poff("conv4.bias"), sp.thin_ws,
                            N, H, W, 1, 64, False),
            ops.image_to_features(dtc, sp.thin_o, sp.dl, V(gA), w4raw, wptr + O[("b", "conv4")], N, H, W, 1, 64, False, flip=True,
                                  mask=V(sp.c3), mask_slope=0.2),
            wg("conv3", sp.c2, gA, H, W, 64, 64, sn_index=7),
            cv(V(gA), V(gB), wptr + O[("b", "conv3")], N, H, W, 64, 64, mask=V(sp.c2), mask_slope=0.2),
            wg("conv2", sp.u3, gB, H, W, 64, 64, sn_index=6),
            # u3 = lrelu(z3) + out1: the conv's two outputs are d u3 (y2: the skip's share, added into d out1 below) and
            # d z3 = d u3 * lrelu'(a3) (y, after the mask) -- no separate LeakyReLU-backward pass over the 512^2 tensor
            cv(V(gB), V(gD), wptr + O[("b", "conv2")], N, H, W, 64, 64, y2=V(gA), mask=V(sp.a3), mask_slope=0.2),   # gA = d u3, gD = d z3
            wg("up_block3", sp.b1, gD, H, W, 128, 64, sn_index=5),
            cv(V(gD), V(gC), wptr + O[("b", "up_block3")], N, H, W, 64, 128),            # gC = d b1
            rsl(V(gC), V(h1), V(sp.a2), V(h2), H // 2, W // 2, 128),                     # h1 = d u2, h2 = d z2
            wg("up_block2", sp.b2, h2, H // 2, W // 2, 256, 128, sn_index=4),
            cv(V(h2), V(h3), wptr + O[("b", "up_block2")], N, H // 2, W // 2, 128, 256),  # h3 = d b2
            rsl(V(h3), V(q1), V(sp.a1), V(q2), H // 4, W // 4, 256),                     # q1 = d u1, q2 = d z1
            wg("up_block1", sp.b3, q2, H // 4, W // 4, 512, 256, sn_index=3),
            cv(V(q2), V(q3), wptr + O[("b", "up_block1")], N, H // 4, W // 4, 256, 512),  # q3 = d b3
            rsl(V(q3), A.NULL_VIEW, V(sp.d3), V(e1), H // 8, W // 8, 512),               # e1 = d d3 (pre-activation)
            wg("down_block3", sp.d2, e1, H // 4, W // 4, 256, 512, sn_index=2, k=4, s=2),
        ]
        bw += s2_dgrad("down_block3", e1, q4, H // 8, W // 8, 512, 256, q1, sp.d2)       # q4 = (d d2 + d u1) * lrelu'(d2)
        bw.append(wg("down_block2", sp.d1, q4, H // 2, W // 2, 128, 256, sn_index=1, k=4, s=2))
        bw += s2_dgrad("down_block2", q4, h4, H // 4, W // 4, 256, 128, h1, sp.d1)       # h4 = (d d1 + d u2) * lrelu'(d1)
        bw.append(wg("down_block1", sp.out1, h4, H, W, 64, 128, sn_index=0, k=4, s=2))
        bw += s2_dgrad("down_block1", h4, gD, H // 2, W // 2, 128, 64, gA, None)         # gD = d out1 (+ skip d u3)
        bw.append(ops.image_wgrad(dtc, sp.thin_i, wplans, sp.xin, gD, w1raw, self._poff("conv1.weight"), self._poff("conv1.bias"), sp.thin_ws,
                                  N, H, W, self.in_ch, 64, True))
        sp.dx_conv = first_layer_dgrad(ops.features_to_image(dtc, sp.thin_i, V(gD), sp.dxp, 4, w1raw, wptr + O[("b", "conv1")], N, H, W, self.in_ch, 64,
                                                             True, flip=True))
        sp.bw = bw
        self._backward_workspaces(sp, wplans, pk)


def discriminator_engine(owner: nn.Module) -> DiscriminatorEngine:
    return _engine(owner, lambda: DiscriminatorEngine(owner))


def discriminator_apply(owner: nn.Module, x: Tensor) -> Tensor:
    return engine_apply(discriminator_engine(owner), x, owner.training)
