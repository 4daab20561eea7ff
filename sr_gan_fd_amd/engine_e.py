"""HIP engine for ESRGAN's VGG-style discriminator.

Reference: Discriminator ESRGAN/model.py:88-141 -- conv3x3(bias) + LeakyReLU, nine (conv without bias, BatchNorm2d,
LeakyReLU(0.2)) stages alternating 4x4 stride 2 / 3x3 stride 1 (3x128x128 -> 512x4x4), flatten, Linear(8192,100),
LeakyReLU, Linear(100,1).

The relativistic step of ESRGAN/train_esrgan.py:395-418 keeps up to three training forwards alive at once (gt_output and
sr_output both feed each loss term, ``backward(retain_graph=True)``), each with its own BatchNorm batch statistics, so
activations live in a ring of RING plan instances per input shape instead of one.

Mapping: the convs are the implicit-GEMM kernel (4x4 stride-2 data gradients as four output-parity classes); BatchNorm +
LeakyReLU is one fused statistics/apply pass per stage (srganfd_batchnorm_act_fwd / _bwd, channel blocks of 256);
``torch.flatten`` of an NCHW tensor followed by Linear(8192,100) IS a 4x4 "valid" convolution of the 4x4x512 map with
the weight viewed as (100,512,4,4) -- same bytes -- so the classifier runs on the conv / wgrad kernels too (4x4 stride 2
without padding, one output pixel per image), and Linear(100,1) is a 1x1 conv.  No transposes, no separate GEMM.
"""
from __future__ import annotations

import weakref

import torch
from torch import Tensor, nn

from . import _abi as A
from . import ops
from .engine import _engine, _Shape, engine_apply
from .engine_core import DiscriminatorEngineCore, first_layer_dgrad

CONV_IDX = (0, 2, 5, 8, 11, 14, 17, 20, 23, 26)          # positions of the convs inside `features`
SLOPE = 0.2
RING = 4                                                   # activation sets per input shape (live forwards of one iteration)


class StageBatchNorm:
    """BatchNorm2d + LeakyReLU of one stage as one fused pass: the conv's output y -> the activation a, ``npix`` pixels of ``channels``.
    ``gamma_off`` / ``beta_off``: elements of the flat parameters and gradient; ``bn``: the module (running buffers, momentum, eps, batch
    counter); ``save``: the statistics the backward pass needs; ``ws``: the plan's statistics workspace"""
    kind = "bn"

    def __init__(self, eng, y: A.View, a: A.View, dtc: int, npix: int, channels: int, gamma_off: int, beta_off: int, bn: nn.Module, save: Tensor, ws: Tensor):
        self.eng, self.y, self.a, self.dtc, self.npix, self.channels = weakref.proxy(eng), y, a, dtc, npix, channels     # (a plan must not hold its engine)
        self.gamma_off, self.beta_off, self.bn, self.save, self.ws = gamma_off, beta_off, bn, save, ws

    def launch(self, run: ops.Run) -> None:
        bn = self.bn
        if bn.running_mean.device != self.ws.device:
            raise A.SrganfdError("BatchNorm buffers must live on the module's GPU")
        flat = self.eng.fp.flat.data_ptr()
        A.check(run.L.srganfd_batchnorm_act_fwd(self.y, self.a, self.dtc, self.npix, self.channels, flat + 4 * self.gamma_off, flat + 4 * self.beta_off,
                                                bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.momentum, bn.eps,
                                                1 if run.training else 0, self.save.data_ptr(), self.ws.data_ptr(), SLOPE, run.st), "batchnorm_act_fwd")
        if run.training:
            bn.num_batches_tracked += 1


class StageBatchNormBwd:
    """backward of the StageBatchNorm ``fwd``: dA (w.r.t. the post-activation) -> dY (w.r.t. the conv output); dgamma / dbeta into the
    pass's flat gradient"""
    kind = "bn_bwd"

    def __init__(self, fwd: StageBatchNorm, dA: A.View, dY: A.View):
        self.fwd, self.dA, self.dY = fwd, dA, dY

    def launch(self, run: ops.Run) -> None:
        f = self.fwd
        gamma, beta = 4 * f.gamma_off, 4 * f.beta_off
        A.check(run.L.srganfd_batchnorm_act_bwd(f.y, self.dA, self.dY, f.dtc, f.npix, f.channels, f.eng.fp.flat.data_ptr() + gamma, f.save.data_ptr(),
                                                run.grad + gamma, run.grad + beta, 0.0, f.ws.data_ptr(), f.a, SLOPE, run.st), "batchnorm_act_bwd")


class EsrganDiscriminatorEngine(DiscriminatorEngineCore):
    what = "Discriminator"
    batch_stats = True

    def __init__(self, owner: nn.Module):
        super().__init__(owner, 3)             # no spectral norm: the pack table simply runs on every forward
        self.convs = []            # (features index, cin, cout, ksize, stride)
        for fi in CONV_IDX:
            m = owner.features[fi]
            self.convs.append((fi, m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0]))
        if self.convs[0][1] != 3 or owner.classifier[0].in_features != 512 * 16 or owner.classifier[2].out_features != 1:
            raise A.SrganfdError("Discriminator: unexpected layer sizes (ESRGAN/model.py:88-141)")
        self.hid = owner.classifier[0].out_features            # 100
        self.hid_pad = ops.pad32(self.hid)
        self._fw_count = 0                                     # forwards so far: picks the plan of the ring

    def _build_pack(self, dtc, device):
        pb = ops.PackBuilder(dtc)

        def layer(key, src, co, ci, ks, stride):
            pb.fwd(("f", key), src, co, ci, ks)
            if stride == 1:
                pb.bwd(("b", key), src, co, ci, ks)
            else:
                pb.classes(("b", key), src, co, ci, 2, 2)
        for fi, ci, co, ks, st in self.convs:
            layer(fi, self._poff(f"features.{fi}.weight"), co, ci, ks, st)
        layer("fc1", self._poff("classifier.0.weight"), self.hid, 512, 4, 2)          # Linear(8192,100) == conv 4x4 over the 4x4 map
        layer("fc2", self._poff("classifier.2.weight"), 1, self.hid, 1, 1)
        return pb.finish(device)

    # ---- per-shape plan: one of a ring of RING per shape, the next one at every forward ----
    def _plan(self, *args):
        self._fw_count += 1
        return super()._plan(*args)

    def _plan_key(self) -> tuple:
        return (self._fw_count % RING,)

    def _plan_forward(self, sp: _Shape, b: ops.PlanBuilder, train: bool) -> None:
        N, V = sp.N, A.view
        lre = dict(act=A.ACT_LRELU, slope=SLOPE)
        sp.xin = b.act(sp.H, sp.W, 32)
        sp.y, sp.a, sp.save, sp.hw, sp.bn = {}, {}, {}, {}, {}
        sp.bn_ws = b.buf(2048 * 256 + 3 * 256, dtype=torch.float32)
        h, w = sp.H, sp.W
        fw = []
        prev = sp.xin
        for i, (fi, ci, co, ks, st) in enumerate(self.convs):
            ho, wo = h // st, w // st
            sp.hw[i] = (h, w, ho, wo)
            sp.a[i] = b.act(ho, wo, co)
            if i == 0:
                fw.append(b.conv(prev, sp.a[0], ("f", fi), h, w, 32, co, bias=b.P("features.0.bias"), **lre))
            else:
                sp.y[i] = b.act(ho, wo, co)
                sp.save[i] = b.buf(4 * co, dtype=torch.float32)
                fw.append(b.conv(prev, sp.y[i], ("f", fi), h, w, ci, co, ksize=ks, stride=st))
                sp.bn[i] = StageBatchNorm(self, V(sp.y[i]), V(sp.a[i]), sp.dtc, N * ho * wo, co, self._poff(f"features.{fi + 1}.weight"),
                                          self._poff(f"features.{fi + 1}.bias"), self.owner.features[fi + 1], sp.save[i], sp.bn_ws)
                fw.append(sp.bn[i])
            prev, h, w = sp.a[i], ho, wo
        sp.f1 = torch.zeros(N, 1, 1, self.hid_pad, dtype=sp.dt, device=sp.device)          # padded channels stay zero (they meet zero weights in fc2)
        fw.append(b.conv(sp.a[9], sp.f1, ("f", "fc1"), 4, 4, 512, self.hid_pad, cout_store=self.hid, ksize=4, stride=2, pad=0,
                         bias=b.P("classifier.0.bias"), **lre))
        # Linear(100,1) writes the logits, allocated per forward
        fw.append(ops.PerCall(b.conv(sp.f1, A.View(0, 1, 0), ("f", "fc2"), 1, 1, self.hid_pad, 32, cout_store=1, ksize=1, pad=0,
                                     bias=b.P("classifier.2.bias"), y_f32=True)))
        sp.fw = fw

    def _plan_backward(self, sp: _Shape, b: ops.PlanBuilder) -> None:
        V = A.view
        sp.dl = b.act(1, 1, 32)
        df1 = b.act(1, 1, self.hid_pad)
        bw = [
            b.wgrad(sp.f1, sp.dl, 1, 1, self.hid_pad, 32, "classifier.2.weight", "classifier.2.bias", cin_real=self.hid, cout_real=1, ksize=1, stride=1, pad=0),
            b.dgrad(sp.dl, df1, ("b", "fc2"), 1, 1, 32, self.hid_pad, mask=sp.f1, mask_slope=SLOPE, ksize=1, pad=0),
            b.wgrad(sp.a[9], df1, 4, 4, 512, self.hid_pad, "classifier.0.weight", "classifier.0.bias", cout_real=self.hid, ksize=4, stride=2, pad=0),
        ]
        dA = b.act(4, 4, 512)                     # gradient w.r.t. a9 (post-activation): the BN backward applies LeakyReLU'
        # the classifier's 4x4 'valid' conv as 4 output-parity classes: 2 x 2 outputs each, the tap pairs of the opposite parity
        bw += b.strided_dgrad(df1, dA, ("b", "fc1"), 1, 1, self.hid_pad, 512, 2, 1, valid=True)
        sp.keep = [df1, dA]
        for i in range(9, 0, -1):
            fi, ci, co, ks, st = self.convs[i]
            h, w, ho, wo = sp.hw[i]
            dY = b.act(ho, wo, co)
            bw.append(StageBatchNormBwd(sp.bn[i], V(dA), V(dY)))
            bw.append(b.wgrad(sp.a[i - 1], dY, h, w, ci, co, f"features.{fi}.weight", ksize=ks, stride=st, pad=1))
            dAp = b.act(h, w, ci)
            # below stage 1 sits conv0 + LeakyReLU (no BatchNorm): its activation derivative goes into this epilogue
            mask0 = sp.a[0] if i == 1 else None
            if st == 1:
                bw.append(b.dgrad(dY, dAp, ("b", fi), ho, wo, co, ci, mask=mask0, mask_slope=SLOPE))
            else:
                bw += b.strided_dgrad(dY, dAp, ("b", fi), ho, wo, co, ci, 2, 1, mask=mask0)      # 4x4 stride 2 pad 1: 2x2-tap classes over dY
            sp.keep += [dY, dAp]
            dA = dAp
        # dA is now dL/d(conv0 output before LeakyReLU)
        bw.append(b.wgrad(sp.xin, dA, sp.H, sp.W, 32, 64, "features.0.weight", "features.0.bias", cin_real=3))
        sp.bw = bw
        sp.dxp = b.act(sp.H, sp.W, 4, dtype=torch.float32)
        sp.dx_conv = first_layer_dgrad(b.conv(dA, sp.dxp, ("b", 0), sp.H, sp.W, 64, 32, cout_store=3, y_f32=True))
        self._backward_workspaces(sp, b)
        sp.per_call = (sp.N, 1)                   # the classifier's logits: no height and width

    # ---- execution: EngineBase's passes ----
    def _check_input(self, x: Tensor):
        dims = super()._check_input(x)
        if tuple(x.shape[2:]) != (128, 128):
            raise A.SrganfdError(f"Discriminator expects 3x128x128 inputs: its classifier is Linear(512*4*4, 100) (ESRGAN/model.py:129); "
                                 f"got shape {tuple(x.shape)}")
        return dims


def esrgan_discriminator_engine(owner: nn.Module) -> EsrganDiscriminatorEngine:
    return _engine(owner, lambda: EsrganDiscriminatorEngine(owner))


def esrgan_discriminator_apply(owner: nn.Module, x: Tensor) -> Tensor:
    return engine_apply(esrgan_discriminator_engine(owner), x, owner.training)
