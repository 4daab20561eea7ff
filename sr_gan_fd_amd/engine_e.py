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

    # ---- per-shape plan ----
    def _plan(self, N, H, W, dt, dtc, device, pk, train=True):
        self._fw_count += 1
        key = (N, H, W, dtc, str(device), pk["buf"].data_ptr(), self.fp.flat.data_ptr(), self._fw_count % RING)
        sp = self.shapes.get(key)
        if sp is not None:
            return sp
        sp = _Shape()
        sp.N, sp.H, sp.W, sp.dt, sp.dtc, sp.device = N, H, W, dt, dtc, device
        V = A.view
        fptr, wptr, O = self.fp.flat.data_ptr(), pk["buf"].data_ptr(), pk["offs"]

        def new(h, w, c, dtype=dt, zero=False):
            f = torch.zeros if zero else torch.empty
            return f(N, h, w, c, dtype=dtype, device=device)
        sp.xin = new(H, W, 32)
        sp.y, sp.a, sp.save, sp.hw, sp.bn = {}, {}, {}, {}, {}
        sp.bn_ws = torch.empty(2048 * 256 + 3 * 256, dtype=torch.float32, device=device)
        h, w = H, W
        fw = []
        cv = lambda *a, **k: ops.Conv(ops.conv_args(dtc, *a, **k))
        prev = sp.xin
        for i, (fi, ci, co, ks, st) in enumerate(self.convs):
            ho, wo = h // st, w // st
            sp.hw[i] = (h, w, ho, wo)
            sp.a[i] = new(ho, wo, co)
            if i == 0:
                fw.append(cv(V(prev), V(sp.a[0]), wptr + O[("f", fi)], N, h, w, 32, co, bias=fptr + 4 * self._poff("features.0.bias"),
                             act=A.ACT_LRELU, slope=SLOPE))
            else:
                sp.y[i] = new(ho, wo, co)
                sp.save[i] = torch.empty(4 * co, dtype=torch.float32, device=device)
                fw.append(cv(V(prev), V(sp.y[i]), wptr + O[("f", fi)], N, h, w, ci, co, ksize=ks, stride=st))
                sp.bn[i] = StageBatchNorm(self, V(sp.y[i]), V(sp.a[i]), dtc, N * ho * wo, co, self._poff(f"features.{fi + 1}.weight"),
                                          self._poff(f"features.{fi + 1}.bias"), self.owner.features[fi + 1], sp.save[i], sp.bn_ws)
                fw.append(sp.bn[i])
            prev, h, w = sp.a[i], ho, wo
        sp.f1 = new(1, 1, self.hid_pad, zero=True)          # padded channels stay zero (they meet zero weights in fc2)
        fw.append(cv(V(sp.a[9]), V(sp.f1), wptr + O[("f", "fc1")], N, 4, 4, 512, self.hid_pad, cout_store=self.hid, ksize=4, stride=2,
                     pad=0, bias=fptr + 4 * self._poff("classifier.0.bias"), act=A.ACT_LRELU, slope=SLOPE))
        # Linear(100,1) writes the logits, allocated per forward
        fw.append(ops.PerCall(cv(V(sp.f1), A.View(0, 1, 0), wptr + O[("f", "fc2")], N, 1, 1, self.hid_pad, 32, cout_store=1, ksize=1, pad=0,
                                 bias=fptr + 4 * self._poff("classifier.2.bias"), y_f32=True)))
        sp.fw = fw
        self._plan_backward(sp, pk)
        self.shapes[key] = sp
        return sp

    def _plan_backward(self, sp, pk):
        N, dt, dtc, device = sp.N, sp.dt, sp.dtc, sp.device
        V = A.view
        wptr, O = pk["buf"].data_ptr(), pk["offs"]

        def new(h, w, c, dtype=dt):
            return torch.empty(N, h, w, c, dtype=dtype, device=device)
        wplans = ops.WgradPlans(device, dtc, N)

        def wg(pname, bname, x, dy, h, w, cin, cout, k, s, pad, cin_real=None, cout_real=None):
            plan = wplans.conv(h, w, cin, cout, self._poff(pname), self._poff(bname) if bname else -1, cin_real, cout_real, ksize=k, stride=s, pad=pad)
            return ops.Wgrad(plan, V(x), V(dy))

        def s2_dgrad(key, dy, dx, hd, wd, cout, cin, mask, pad):
            """data gradient of a 4x4 stride-2 conv as 4 output-parity classes (2x2-tap convs over dy).  pad = 1: class
            (py,px) has hd x wd outputs; pad = 0 (the classifier's 4x4 'valid' conv): hd+1 x wd+1 outputs, the tap pairs of
            the opposite parity and one row/column of zero padding on the low side."""
            return ops.parity_class_launches(
                dtc, V(dy), V(dx), wptr, [O[("b", key, c)] for c in range(4)], N, hd, wd, cout, cin, 2, 1, valid=pad == 0,
                **ops.dgrad_epilogue(mask=None if mask is None else V(mask), mask_slope=SLOPE))

        cv = lambda *a, **k: ops.Conv(ops.conv_args(dtc, *a, **k))
        sp.dl = new(1, 1, 32)
        df1 = new(1, 1, self.hid_pad)
        bw = [
            wg("classifier.2.weight", "classifier.2.bias", sp.f1, sp.dl, 1, 1, self.hid_pad, 32, 1, 1, 0, cin_real=self.hid, cout_real=1),
            cv(V(sp.dl), V(df1), wptr + O[("b", "fc2")], N, 1, 1, 32, self.hid_pad, ksize=1, pad=0, mask=V(sp.f1), mask_slope=SLOPE),
            wg("classifier.0.weight", "classifier.0.bias", sp.a[9], df1, 4, 4, 512, self.hid_pad, 4, 2, 0, cout_real=self.hid),
        ]
        dA = new(4, 4, 512)                       # gradient w.r.t. a9 (post-activation): the BN backward applies LeakyReLU'
        bw += s2_dgrad("fc1", df1, dA, 1, 1, self.hid_pad, 512, None, 0)
        sp.keep = [df1, dA]
        for i in range(9, 0, -1):
            fi, ci, co, ks, st = self.convs[i]
            h, w, ho, wo = sp.hw[i]
            dY = new(ho, wo, co)
            bw.append(StageBatchNormBwd(sp.bn[i], V(dA), V(dY)))
            xprev = sp.a[i - 1]
            bw.append(wg(f"features.{fi}.weight", None, xprev, dY, h, w, ci, co, ks, st, 1))
            dAp = new(h, w, ci)
            # below stage 1 sits conv0 + LeakyReLU (no BatchNorm): its activation derivative goes into this epilogue
            mask0 = sp.a[0] if i == 1 else None
            if st == 1:
                bw.append(cv(V(dY), V(dAp), wptr + O[("b", fi)], N, ho, wo, co, ci, mask=V(mask0) if mask0 is not None else A.NULL_VIEW,
                             mask_slope=SLOPE))
            else:
                bw += s2_dgrad(fi, dY, dAp, ho, wo, co, ci, mask0, 1)
            sp.keep += [dY, dAp]
            dA = dAp
        # dA is now dL/d(conv0 output before LeakyReLU)
        bw.append(wg("features.0.weight", "features.0.bias", sp.xin, dA, sp.H, sp.W, 32, 64, 3, 1, 1, cin_real=3))
        sp.bw = bw
        sp.dxp = torch.empty(N, sp.H, sp.W, 4, dtype=torch.float32, device=device)
        sp.dx_conv = first_layer_dgrad(cv(V(dA), V(sp.dxp), wptr + O[("b", 0)], N, sp.H, sp.W, 64, 32, cout_store=3, y_f32=True))
        self._backward_workspaces(sp, wplans, pk)
        sp.per_call = (N, 1)                      # the classifier's logits: no height and width

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
