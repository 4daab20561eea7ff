"""HIP engine of A-ESRGAN's pixel-attention generator (A-ESRGAN/model.py:87-175): one engine class for a lone ``RPA``, a lone ``US``
and the whole ``Generator_RPA``, which is a list of such blocks between a head (conv1) and a tail (conv2, conv3).  The class checks
the module, packs its weights and plans the launch lists; running them, the layout conversions at both ends of a pass and the
autograd glue are engine.py's (EngineBase).

Every convolution is a launch of the implicit-GEMM kernel (1x1 and 3x3, forward, data gradient, weight-gradient plans); the one thing
no existing kernel does, ``z = x * (1 + sigmoid(a))`` and its backward, is srganfd_pixel_gate (csrc/pixel_gate.hip).

Forward (F = num_feat; every conv adds its bias; ``lrelu`` = LeakyReLU(0.2) in the conv's epilogue)
  RPA(x)   h1 = lrelu(conv1 1x1 F -> 2F (x)), h2 = lrelu(conv2 1x1 2F -> 4F (h1)), a = conv3 3x3 4F -> F (h2),
           g = pixel_gate(x, a), y = lrelu(conv4 3x3 F -> F (g))
  US(x)    u = lrelu(conv1 1x1 (x)), a = pa_conv 1x1 (u), g = pixel_gate(u, a), y = lrelu(conv2 3x3 (nearest_x2(g)))
           THE ONE ALGEBRAIC REWRITE: the reference upsamples x first (model.py:102).  1x1 convs, LeakyReLU, sigmoid and the gate act
           per pixel, so they commute with nearest-neighbour replication value for value: conv1, pa_conv and the gate run at the LOW
           resolution -- a quarter of the reference's work -- and conv2 gathers its input through the conv's fused nearest-x2 read
           (srganfd_conv_args.up = 1).
  Generator_RPA(x)   z0 = lrelu(conv1 3x3 in -> F (x)) (ops.image_to_features: the thin kernel in 16-bit, padded igemm in fp32), the RPA
           chain, s = z0 + y_last (the last RPA's conv4 adds z0 as r1 and keeps y_last, the LeakyReLU output, as its second output y2
           for the backward's mask), ceil(log2(scale)) US blocks, c2 = lrelu(conv2 3x3 F -> F/2), out = conv3 3x3 F/2 -> out (padded
           to 32 output channels, cout_store = out, fp32).
Backward: the mirror image.  Every conv has a weight-gradient launch and a data-gradient conv whose epilogue multiplies by the
  LeakyReLU derivative of the layer below (``mask``); pixel_gate(bwd) turns dg into da (in place) and the gate's direct gradient,
  which joins the data gradient of the block's first 1x1 conv as r1 at scale 1; in the generator the long skip's gradient ds joins the
  first RPA's the same way (r2) and reaches the last RPA through srganfd_lrelu_bwd; a US block sums the high-resolution data gradient
  of conv2 over each 2x2 cell (srganfd_resample op 0) before the gate.

Rounding points in the 16-bit modes (the oracle, tests/rpa_oracle.py, rounds at exactly these): the input, every packed weight, every
stored activation (h1, h2, a, g, y; u; z0, s, c2 -- s is rounded once from the fp32 sum, y_last separately), and every stored gradient:
d out, the gradient of every conv's pre-activation (after the mask), dg (in a US block twice: at the high resolution and after the 2x2
sum), da, the gate's direct gradient, ds.  Biases, accumulations, the output and the gradients handed to torch are fp32; a lone block's
output is its stored y widened to fp32.
"""
from __future__ import annotations

import math
from typing import Tuple

import torch
from torch import Tensor, nn

from . import _abi as A
from . import ops
from .engine import EngineBase, _engine, _Shape, engine_apply
from .engine_core import first_layer_dgrad

WHAT = {"rpa": "RPA", "us": "US", "gen": "Generator_RPA"}


def check_features(kind: str, num_feat: int) -> None:
    """what the MFMA convs need of num_feat, checked when the module is built"""
    if kind == "gen" and (num_feat <= 0 or num_feat % 64):
        raise A.SrganfdError(f"Generator_RPA: num_feat {num_feat} must be a multiple of 64 (conv2 writes num_feat // 2 channels, a multiple of 32 "
                             "for the MFMA convs)")
    if num_feat <= 0 or num_feat % 32:
        raise A.SrganfdError(f"{WHAT[kind]}: num_feat {num_feat} must be a multiple of 32 for the MFMA convs")


class RpaEngine(EngineBase):
    def __init__(self, owner: nn.Module, kind: str):
        super().__init__(owner, list(owner.named_parameters()))
        self.kind, self.what, self.gen = kind, WHAT[kind], kind == "gen"
        if self.gen:
            self.F, self.in_ch, self.out_ch = owner.conv1.weight.shape[0], owner.conv1.weight.shape[1], owner.conv3.weight.shape[0]
            self.blocks = [("rpa", f"rpa.{n}.") for n, _ in owner.rpa.named_children()] + [("us", f"us.{n}.") for n, _ in owner.us.named_children()]
            self.n_rpa = len(owner.rpa)
            if self.n_rpa < 1:
                raise A.SrganfdError("Generator_RPA: num_block must be at least 1")
            if not (1 <= self.in_ch <= 32 and 1 <= self.out_ch <= 4):
                raise A.SrganfdError(f"Generator_RPA: {self.in_ch} input / {self.out_ch} output channels have no kernel (1..32 in, 1..4 out)")
        else:
            self.F = self.in_ch = self.out_ch = owner.conv1.weight.shape[1]
            self.blocks, self.n_rpa = [(kind, "")], 1 if kind == "rpa" else 0
        check_features(kind, self.F)
        for m in ([owner] if kind == "us" else (list(owner.us) if self.gen else [])):
            if m.scale != 2:
                raise A.SrganfdError(f"US: scale {m.scale} has no kernel (nearest x2 only)")

    def _convs(self):
        """(parameter prefix, cout, cin, ksize) of every conv on the implicit-GEMM kernel"""
        F = self.F
        for kind, pre in self.blocks:
            if kind == "rpa":
                yield from ((pre + "conv1", 2 * F, F, 1), (pre + "conv2", 4 * F, 2 * F, 1), (pre + "conv3", F, 4 * F, 3), (pre + "conv4", F, F, 3))
            else:
                yield from ((pre + "conv1", F, F, 1), (pre + "pa_conv", F, F, 1), (pre + "conv2", F, F, 3))
        if self.gen:
            yield from (("conv1", F, self.in_ch, 3), ("conv2", F // 2, F, 3), ("conv3", self.out_ch, F // 2, 3))

    def _build_pack(self, dtc: int, device) -> dict:
        pb = ops.PackBuilder(dtc)
        for name, co, ci, k in self._convs():
            pb.fwd(("f", name), self._poff(name + ".weight"), co, ci, k)
            pb.bwd(("b", name), self._poff(name + ".weight"), co, ci, k)
        return pb.finish(device)

    # ---- per-shape plan ----
    def _plan_forward(self, sp: _Shape, b: ops.PlanBuilder, train: bool) -> None:
        N, H, W, dtc, F, V = sp.N, sp.H, sp.W, sp.dtc, self.F, A.view
        lre = dict(act=A.ACT_LRELU, slope=0.2)
        shared = {}

        def act(role, bi, h, w, c):
            """a block's activation buffer: its own when a backward pass will read it; an inference plan shares one per role among the
            blocks (they run one after the other), block outputs alternating between two"""
            if train:
                return b.act(h, w, c)
            k = (role if role != "y" else "y%d" % (bi & 1), h, w, c)
            if k not in shared:
                shared[k] = b.act(h, w, c)
            return shared[k]

        def layer(x, y, name, h, w, cin, cout, k, **kw):
            """conv ``name`` (k x k, 'same' padding) with its bias"""
            return b.conv(x, y, ("f", name), h, w, cin, cout, ksize=k, pad=k // 2, bias=b.P(name + ".bias"), **kw)

        def gate(h, w, x, a, z):
            return ops.PixelGate(ops.pixel_gate_args(dtc, N * h * w, F, V(x), V(a), z=V(z)))
        fw = []
        if self.gen:
            sp.thin_i = ops.thin_ok(dtc, F, self.in_ch)
            sp.xin, sp.z0 = b.act(H, W, 4 if sp.thin_i else 32), b.act(H, W, F)
            fw.append(b.image_to_features(sp.thin_i, sp.xin, sp.z0, "conv1", H, W, self.in_ch, F, True, **lre))
            cur = sp.z0
        else:
            sp.xin = cur = b.act(H, W, F)
        h, w = H, W
        sp.recs = []
        for bi, (kind, pre) in enumerate(self.blocks):
            r = _Shape()
            r.kind, r.pre, r.h, r.w, r.x = kind, pre, h, w, cur
            if kind == "rpa":
                r.h1, r.h2, r.a, r.g, r.y = act("h1", bi, h, w, 2 * F), act("h2", bi, h, w, 4 * F), act("a", bi, h, w, F), act("g", bi, h, w, F), act("y", bi, h, w, F)
                fw += [layer(r.x, r.h1, pre + "conv1", h, w, F, 2 * F, 1, **lre), layer(r.h1, r.h2, pre + "conv2", h, w, 2 * F, 4 * F, 1, **lre),
                       layer(r.h2, r.a, pre + "conv3", h, w, 4 * F, F, 3), gate(h, w, r.x, r.a, r.g)]
                if self.gen and bi == self.n_rpa - 1:
                    # the long skip z + z_ (model.py:170) in the last RPA's conv4: s = z0 + lrelu(...), the LeakyReLU output kept beside it
                    sp.s = b.act(h, w, F)
                    fw.append(layer(r.g, sp.s, pre + "conv4", h, w, F, F, 3, r1=V(sp.z0), r1_scale=1.0, y2=V(r.y), **lre))
                    cur = sp.s
                else:
                    fw.append(layer(r.g, r.y, pre + "conv4", h, w, F, F, 3, **lre))
                    cur = r.y
            else:
                r.u, r.a, r.g, r.y = act("u", bi, h, w, F), act("a", bi, h, w, F), act("g", bi, h, w, F), act("y", bi, 2 * h, 2 * w, F)
                fw += [layer(r.x, r.u, pre + "conv1", h, w, F, F, 1, **lre), layer(r.u, r.a, pre + "pa_conv", h, w, F, F, 1), gate(h, w, r.u, r.a, r.g),
                       layer(r.g, r.y, pre + "conv2", h, w, F, F, 3, up=1, **lre)]
                cur, h, w = r.y, 2 * h, 2 * w
            sp.recs.append(r)
        if self.gen:
            sp.c2, sp.srp = b.act(h, w, F // 2), b.act(h, w, 4, dtype=torch.float32)
            fw.append(layer(cur, sp.c2, "conv2", h, w, F, F // 2, 3, **lre))
            fw.append(b.conv(sp.c2, sp.srp, ("f", "conv3"), h, w, F // 2, 32, cout_store=self.out_ch, bias=b.P("conv3.bias"), y_f32=True))
        sp.fw, sp.last, sp.hs, sp.ws = fw, cur, h, w
        sp.x_in = (V(sp.xin), sp.xin.shape[-1])
        sp.result = (V(sp.srp), A.F32, 0) if self.gen else (V(cur), dtc, 0)      # (a lone block: its stored y, widened)

    def _plan_backward(self, sp: _Shape, b: ops.PlanBuilder) -> None:
        N, H, W, dtc, F, V = sp.N, sp.H, sp.W, sp.dtc, self.F, A.view
        hs, ws = sp.hs, sp.ws
        pool, turn = {}, [0]
        bw = []

        def gb(h, w, c, slot):
            """the blocks run one after the other and share their gradient buffers by role"""
            k = (h, w, c, slot)
            if k not in pool:
                pool[k] = b.act(h, w, c)
            return pool[k]

        def pre_buf(h, w):
            """gradients of a block's last pre-activation alternate between two buffers: a block reads one and writes the other"""
            turn[0] ^= 1
            return gb(h, w, F, "pre%d" % turn[0])

        def layer_bwd(name, x, dy, dx, h, w, cin, cout, k, up=0, **epilogue):
            """weight gradient of conv ``name`` (x: its input, dy: its pre-activation's gradient at (h << up, w << up)) and its data
            gradient into dx with ``epilogue`` (PlanBuilder.dgrad's r1 / r2 / mask / y_f32)"""
            bw.append(b.wgrad(x, dy, h, w, cin, cout, name + ".weight", name + ".bias", ksize=k, pad=k // 2, up=up))
            return b.dgrad(dy, dx, ("b", name), h << up, w << up, cout, cin, ksize=k, pad=k // 2, **epilogue)

        def gate(h, w, x, a, dz, dx):
            return ops.PixelGate(ops.pixel_gate_args(dtc, N * h * w, F, V(x), V(a), dz=V(dz), dx=V(dx), da=V(dz)))       # da over dz, in place

        def through_skip():
            """ds is complete: the last RPA's share of it, times the LeakyReLU derivative of that block's output"""
            dpre = pre_buf(H, W)
            bw.append(b.lrelu_bwd(sp.ds, sp.recs[self.n_rpa - 1].y, dpre, N * H * W, F))
            return dpre
        if self.gen:
            sp.dout = b.act(hs, ws, 32)
            sp.ds = b.act(H, W, F)
            dc2 = gb(hs, ws, F // 2, "dc2")
            bw.append(b.wgrad(sp.c2, sp.dout, hs, ws, F // 2, 32, "conv3.weight", "conv3.bias", cout_real=self.out_ch))
            bw.append(b.dgrad(sp.dout, dc2, ("b", "conv3"), hs, ws, 32, F // 2, mask=sp.c2))
            if self.blocks[-1][0] == "us":
                dpre = pre_buf(hs, ws)
                bw.append(layer_bwd("conv2", sp.last, dc2, dpre, hs, ws, F, F // 2, 3, mask=sp.last))
            else:
                bw.append(layer_bwd("conv2", sp.last, dc2, sp.ds, hs, ws, F, F // 2, 3))
                dpre = through_skip()
        else:
            sp.dout = b.act(hs, ws, F)
            dpre = pre_buf(hs, ws)
            bw.append(b.lrelu_bwd(sp.dout, sp.last, dpre, N * hs * ws, F))
        sp.dx_conv = None
        for bi in range(len(self.blocks) - 1, -1, -1):
            r = sp.recs[bi]
            kind, pre, h, w = r.kind, r.pre, r.h, r.w
            dz, dxg = gb(h, w, F, "dz"), gb(h, w, F, "dxg")
            if kind == "rpa":
                dh2, dh1 = gb(h, w, 4 * F, "dh2"), gb(h, w, 2 * F, "dh1")
                bw.append(layer_bwd(pre + "conv4", r.g, dpre, dz, h, w, F, F, 3))
                bw.append(gate(h, w, r.x, r.a, dz, dxg))
                bw.append(layer_bwd(pre + "conv3", r.h2, dz, dh2, h, w, 4 * F, F, 3, mask=r.h2))
                bw.append(layer_bwd(pre + "conv2", r.h1, dh2, dh1, h, w, 2 * F, 4 * F, 1, mask=r.h1))
                first = dict(dy=dh1, cout=2 * F, r1=dxg)
            else:
                dghi, du = gb(2 * h, 2 * w, F, "dghi"), gb(h, w, F, "du")
                bw.append(layer_bwd(pre + "conv2", r.g, dpre, dghi, h, w, F, F, 3, up=1))
                bw.append(b.resample(0, dghi, dz, h, w, F, what="nearest_bwd"))
                bw.append(gate(h, w, r.u, r.a, dz, dxg))
                bw.append(layer_bwd(pre + "pa_conv", r.u, dz, du, h, w, F, F, 1, r1=dxg, mask=r.u))
                first = dict(dy=du, cout=F, r1=None)
            # the block's first conv: where its data gradient goes and what joins it depends on what the block's input is
            conv1 = lambda dx, **epilogue: layer_bwd(pre + "conv1", r.x, first["dy"], dx, h, w, F, first["cout"], 1, r1=first["r1"], **epilogue)
            if not self.gen:                      # a lone block: the module's input, fp32, launched only when its gradient is wanted
                sp.dxp = b.act(H, W, F, dtype=torch.float32)
                sp.dx_conv = conv1(sp.dxp, y_f32=True)
            elif r.x is sp.s:                     # the sum z0 + y_last: no activation of its own
                bw.append(conv1(sp.ds))
                dpre = through_skip()
            else:                                 # a LeakyReLU output: the previous block's, or (first RPA) conv1's, which the long skip also reads
                nxt = pre_buf(h, w)
                bw.append(conv1(nxt, r2=sp.ds if bi == 0 else None, mask=r.x))
                dpre = nxt
        if self.gen:
            sp.thin_ws = b.thin_ws(sp.thin_i)
            bw.append(b.image_wgrad(sp.thin_i, sp.xin, dpre, "conv1", sp.thin_ws, H, W, self.in_ch, F, True))
            sp.dxp = b.act(H, W, 4, dtype=torch.float32)
            sp.dx_conv = first_layer_dgrad(b.features_to_image(sp.thin_i, dpre, sp.dxp, 4, "conv1", H, W, self.in_ch, F, True, flip=True))
        sp.pool, sp.wg_ws, sp.bw = pool, b.wplans.workspace(), bw
        sp.dy_in, sp.dx_out = (V(sp.dout), sp.dout.shape[-1]), (V(sp.dxp), A.F32)

    # ---- execution ----
    def output_shape(self, shape) -> Tuple[int, int, int, int]:
        N, _, H, W = shape
        up = sum(1 for k, _ in self.blocks if k == "us")
        return (N, self.out_ch, H << up, W << up)


def rpa_engine(owner: nn.Module, kind: str) -> RpaEngine:
    return _engine(owner, lambda: RpaEngine(owner, kind))


def rpa_apply(owner: nn.Module, kind: str, x: Tensor) -> Tensor:
    """forward of RPA / US / Generator_RPA: through autograd when the input or a parameter wants a gradient"""
    return engine_apply(rpa_engine(owner, kind), x)


def num_usblock(scale: int) -> int:
    return math.ceil(math.log2(scale))
