"""HIP engine for the A-ESRGAN attention U-Net discriminator (BASELINE config 5).

Reference: UNetDiscriminatorAesrgan.forward A-ESRGAN/model.py:311-338, add_attn.forward :239-254,
unetCat.forward :265-275, spectral_norm as in engine_d.py.

Data flow (NHWC; R0 = input size, Rk = R0 / 2^k, Rg = R3 + 2):
  x -> conv0 -> x0 -3x3s2-> x1 -3x3s2-> x2 -3x3s2-> x3 -1x1 pad1-> gated (Rg)
  attention gate k on (x2 | x1 | x0): theta = conv2x2s2(x); phi = resize(conv1x1(gated)); f = relu(theta+phi);
      sig = sigmoid(conv1x1(f)) (fp32 map); y = up2(sig) * x; BN(conv1x1(y)) -> channels [0,C) of cat_k
  cat_k channels [C,2C) = lrelu(convU_k(up2(prev)));  x4 = conv4(cat_1) ... x6 = conv6(cat_3) -> conv7 -> conv8 -> conv9
torch.cat never runs (both halves are written into one buffer); the skip/attention gradient sums are folded
into the data-gradient epilogues (two residual inputs + LeakyReLU' mask); the stride-2 3x3 data gradients run
as 4 output-parity classes of 2x2-tap convs, the 2x2 stride-2 ones as 4 classes of 1x1 convs.
"""
from __future__ import annotations

import weakref
import torch
from torch import Tensor, nn

from . import _abi as A
from . import ops
from .engine import _engine, _Shape, engine_apply
from .engine_core import DiscriminatorEngineCore, first_layer_dgrad

# (name, ksize, stride, pad) of the spectral-normalised convs, in forward order
SN_LAYERS = [("conv1", 3, 2, 1), ("conv2", 3, 2, 1), ("conv3", 3, 2, 1), ("gating", 1, 1, 1), ("cat_1.convU", 3, 1, 1),
             ("conv4", 3, 1, 1), ("cat_2.convU", 3, 1, 1), ("conv5", 3, 1, 1), ("cat_3.convU", 3, 1, 1), ("conv6", 3, 1, 1),
             ("conv7", 3, 1, 1), ("conv8", 3, 1, 1)]
SN_INDEX = {n: i for i, (n, _, _, _) in enumerate(SN_LAYERS)}


def _mod(owner: nn.Module, name: str) -> nn.Module:
    m = owner
    for part in name.split("."):
        m = getattr(m, part)
    return m


class GateBatchNorm:
    """BatchNorm2d of an attention gate's W branch, x -> y (its half of the concatenation buffer) over ``npix`` pixels of ``channels``.
    ``gamma_off`` / ``beta_off``: elements of the flat parameters and gradient; ``bn``: the module (running buffers, momentum, eps, batch
    counter); ``save``: the statistics the backward pass needs; ``ws``: what the plan's BatchNorm items share -- [statistics workspace,
    the buffer the sync-BN backward reduces the ranks' sums in (allocated by its first use)]"""
    kind = "bn"

    def __init__(self, eng, x: A.View, y: A.View, dtc: int, npix: int, channels: int, gamma_off: int, beta_off: int, bn: nn.Module, save: Tensor, ws: list):
        self.eng, self.x, self.y, self.dtc, self.npix, self.channels = weakref.proxy(eng), x, y, dtc, npix, channels     # (a plan must not hold its engine)
        self.gamma_off, self.beta_off, self.bn, self.save, self.ws = gamma_off, beta_off, bn, save, ws

    def launch(self, run: ops.Run) -> None:
        bn, L, st, npix, Ck, ws, sb = self.bn, run.L, run.st, self.npix, self.channels, self.ws[0], self.eng.sync_bn
        if bn.running_mean.device != ws.device:
            raise A.SrganfdError("BatchNorm buffers must live on the module's GPU")
        flat = self.eng.fp.flat.data_ptr()
        args = (self.x, self.y, self.dtc, npix, Ck, flat + 4 * self.gamma_off, flat + 4 * self.beta_off, bn.running_mean.data_ptr(), bn.running_var.data_ptr(),
                bn.momentum, bn.eps)
        if run.training and sb is not None:
            # (sum x, sum x^2) of this rank's pixels -> summed over the ranks -> statistics of the whole batch (pixel count = ranks * npix)
            args += (self.save.data_ptr(), ws.data_ptr(), 1.0)
            A.check(L.srganfd_batchnorm_fwd_sync(*args, 1, 0, st), "batchnorm_fwd_sync")
            sb.all_reduce(ws[:L.srganfd_batchnorm_partial_floats(Ck)])
            A.check(L.srganfd_batchnorm_fwd_sync(*args, 2, npix * sb.world, st), "batchnorm_fwd_sync")
        else:
            A.check(L.srganfd_batchnorm_fwd(*args, 1 if run.training else 0, self.save.data_ptr(), ws.data_ptr(), st), "batchnorm_fwd")
        if run.training:
            bn.num_batches_tracked += 1


class GateBatchNormBwd:
    """backward of the GateBatchNorm ``fwd``: dy -> dx; dgamma / dbeta go into the pass's flat gradient"""
    kind = "bn_bwd"

    def __init__(self, fwd: GateBatchNorm, dy: A.View, dx: A.View):
        self.fwd, self.dy, self.dx = fwd, dy, dx

    def launch(self, run: ops.Run) -> None:
        f, L, st = self.fwd, run.L, run.st
        npix, Ck, ws, sb = f.npix, f.channels, f.ws[0], f.eng.sync_bn
        args = (f.x, self.dy, self.dx, f.dtc, npix, Ck, f.eng.fp.flat.data_ptr() + 4 * f.gamma_off, f.save.data_ptr(), run.grad + 4 * f.gamma_off,
                run.grad + 4 * f.beta_off, 0.0, ws.data_ptr())
        if sb is not None:
            # dgamma/dbeta stay this rank's sums (the flat-gradient all-reduce averages them with everything else); the
            # dx coefficients need (sum dy, sum dy*xhat) over the whole batch
            nfl = L.srganfd_batchnorm_partial_floats(Ck)
            if f.ws[1] is None:
                f.ws[1] = torch.empty(L.srganfd_batchnorm_partial_floats(256), dtype=torch.float32, device=ws.device)
            glob = f.ws[1]
            args += (glob.data_ptr(), A.NULL_VIEW, 1.0)
            A.check(L.srganfd_batchnorm_bwd_sync(*args, 1, 0, st), "batchnorm_bwd_sync")
            glob[:nfl].copy_(ws[:nfl])
            sb.all_reduce(glob[:nfl])
            A.check(L.srganfd_batchnorm_bwd_sync(*args, 2, npix * sb.world, st), "batchnorm_bwd_sync")
        else:
            A.check(L.srganfd_batchnorm_bwd(*args, st), "batchnorm_bwd")


class AesrganDiscriminatorEngine(DiscriminatorEngineCore):
    what = "UNetDiscriminatorAesrgan"
    batch_stats = True

    def __init__(self, owner: nn.Module):
        super().__init__(owner, owner.conv0.weight.shape[1], [n + ".weight_orig" for n, _, _, _ in SN_LAYERS])
        self.nf = owner.conv0.weight.shape[0]
        if self.nf != 64:
            raise A.SrganfdError("UNetDiscriminatorAesrgan: num_feat must be 64 (channel counts are multiples of 32, BatchNorm <= 256 channels)")
        self.sync_bn = None   # data parallel: SyncBatchNormReduce -- batch statistics over all ranks (set by GanTrainer(sync_batchnorm=True))

    def _wshape(self, name):
        w = _mod(self.owner, name)
        w = w.weight_orig if hasattr(w, "weight_orig") else w.weight
        return w.shape[0], w.shape[1]

    # ---- packing ----
    def _build_pack(self, dtc, device):
        pb = ops.PackBuilder(dtc)

        def plain(name, ks):
            co, ci = self._wshape(name)
            pb.fwd(("f", name), self._poff(name + ".weight"), co, ci, ks)
            pb.bwd(("b", name), self._poff(name + ".weight"), co, ci, ks)
        plain("conv0", 3)
        plain("conv9", 3)
        for l, (name, ks, st, _) in enumerate(SN_LAYERS):
            co, ci = self._wshape(name)
            src = self._poff(name + ".weight_orig")
            sc = 2 * l + 1
            pb.fwd(("f", name), src, co, ci, ks, scale_off=sc)
            if st == 1:
                pb.bwd(("b", name), src, co, ci, ks, scale_off=sc)
            else:                      # 3x3 stride-2 data gradient: 4 parity classes of 2x2-tap convs
                pb.classes(("b", name), src, co, ci, 2, 6, scale_off=sc)
        for k in (1, 2, 3):
            pre = f"attn_{k}"
            plain(pre + ".W.0", 1)
            plain(pre + ".phi", 1)
            plain(pre + ".psi", 1)
            co, ci = self._wshape(pre + ".theta")
            src = self._poff(pre + ".theta.weight")
            pb.fwd(("f", pre + ".theta"), src, co, ci, 2)
            pb.classes(("b", pre + ".theta"), src, co, ci, 1, 10)      # 2x2 stride-2 data gradient: 4 classes of 1x1 convs
        return pb.finish(device)

    # ---- plan: the buffer tables, the attention gate (forward and backward), the U-Net spine (forward and backward) ----
    def _forward_buffers(self, sp: _Shape, b: ops.PlanBuilder) -> None:
        """sp.B: the spine's activations by name; sp.attn[k]: gate k's (``dims``: its sizes); R[k]: the size at depth k, Rg: the gating map's"""
        H, W, nf = sp.H, sp.W, self.nf
        R = sp.R = [(H >> k, W >> k) for k in range(4)]
        Hg, Wg = sp.Rg = (R[3][0] + 2, R[3][1] + 2)
        B = sp.B = {}
        B["xin"] = sp.xin = b.act(H, W, 4 if sp.thin_i else 32)
        B["x0"], B["x1"], B["x2"], B["x3"] = b.act(*R[0], nf), b.act(*R[1], 2 * nf), b.act(*R[2], 4 * nf), b.act(*R[3], 8 * nf)
        B["gated"] = b.act(Hg, Wg, 4 * nf)
        B["cat1"], B["cat2"], B["cat3"] = b.act(*R[2], 8 * nf), b.act(*R[1], 4 * nf), b.act(*R[0], 2 * nf)
        B["b3"], B["x4"], B["b4"], B["x5"], B["b5"] = b.act(*R[2], 8 * nf), b.act(*R[2], 4 * nf), b.act(*R[1], 4 * nf), b.act(*R[1], 2 * nf), b.act(*R[0], 2 * nf)
        B["x6"], B["c7"], B["c8"] = b.act(*R[0], nf), b.act(*R[0], nf), b.act(*R[0], nf)
        sp.attn = {}
        for k, xname in ((1, "x2"), (2, "x1"), (3, "x0")):
            Ck = B[xname].shape[-1]
            h, w = R[3 - k]
            hh, wh = h // 2, w // 2
            T = sp.attn[k] = {}
            T["theta"], T["phi"], T["phiup"], T["f"] = b.act(hh, wh, Ck), b.act(Hg, Wg, Ck), b.act(hh, wh, Ck), b.act(hh, wh, Ck)
            T["sig"], T["sigup"] = b.act(hh, wh, 1, dtype=torch.float32), b.act(h, w, 1, dtype=torch.float32)
            T["y"], T["wy"] = b.act(h, w, Ck), b.act(h, w, Ck)
            T["save"] = b.buf(4 * Ck, dtype=torch.float32)
            T["dims"] = (h, w, hh, wh, Ck)

    def _backward_buffers(self, sp: _Shape, b: ops.PlanBuilder) -> None:
        """sp.G: the spine's gradients by name; sp.attn[k]["grad"]: gate k's"""
        H, W, nf, R = sp.H, sp.W, self.nf, sp.R
        Hg, Wg = sp.Rg
        sp.dl = b.act(H, W, 4 if sp.thin_o else 32)
        sp.thin_ws = b.thin_ws(sp.thin_i, sp.thin_o)
        G = sp.G = {}
        G["g8"], G["g7"], G["g6"] = b.act(*R[0], nf), b.act(*R[0], nf), b.act(*R[0], nf)
        G["dc3"], G["db5"], G["dx5"] = b.act(*R[0], 2 * nf), b.act(*R[0], 2 * nf), b.act(*R[1], 2 * nf)
        G["dc2"], G["db4"], G["dx4"] = b.act(*R[1], 4 * nf), b.act(*R[1], 4 * nf), b.act(*R[2], 4 * nf)
        G["dc1"], G["db3"], G["dx3a"], G["dx3"] = b.act(*R[2], 8 * nf), b.act(*R[2], 8 * nf), b.act(*R[3], 8 * nf), b.act(*R[3], 8 * nf)
        G["dx2"], G["dx1"], G["dx0"] = b.act(*R[2], 4 * nf), b.act(*R[1], 2 * nf), b.act(*R[0], nf)
        G["dgated"] = [b.act(Hg, Wg, 4 * nf) for _ in range(3)]
        sp.dxp = b.act(H, W, 4, dtype=torch.float32)
        for k in (1, 2, 3):
            h, w, hh, wh, Ck = sp.attn[k]["dims"]
            D = sp.attn[k]["grad"] = {}
            D["dwy"], D["dy"], D["dxg"] = b.act(h, w, Ck), b.act(h, w, Ck), b.act(h, w, Ck)
            D["dsigup"], D["dsig"] = b.act(h, w, 1, dtype=torch.float32), b.act(hh, wh, 1, dtype=torch.float32)
            D["dpsip"], D["df"], D["dxt"], D["dphi"] = b.act(hh, wh, 32), b.act(hh, wh, Ck), b.act(h, w, Ck), b.act(Hg, Wg, Ck)

    def _gate_forward(self, sp: _Shape, b: ops.PlanBuilder, k: int, xname: str, cat: str, bn_ws: list) -> list:
        """attention gate k on the skip B[xname], into channels [0, Ck) of B[cat]"""
        N, dtc, nf, B, V = sp.N, sp.dtc, self.nf, sp.B, A.view
        pre, T = f"attn_{k}", sp.attn[k]
        h, w, hh, wh, Ck = T["dims"]
        Hg, Wg = sp.Rg
        one = dict(ksize=1, pad=0)
        sp.bn[k] = GateBatchNorm(self, V(T["wy"]), V(B[cat]), dtc, N * h * w, Ck, self._poff(pre + ".W.1.weight"), self._poff(pre + ".W.1.bias"),
                                 _mod(self.owner, pre + ".W.1"), T["save"], bn_ws)
        return [
            b.conv(B[xname], T["theta"], ("f", pre + ".theta"), h, w, Ck, Ck, ksize=2, stride=2, pad=0),
            b.conv(B["gated"], T["phi"], ("f", pre + ".phi"), Hg, Wg, 4 * nf, Ck, bias=b.P(pre + ".phi.bias"), **one),
            ops.Call("srganfd_resize_bilinear", (0, V(T["phi"]), V(T["phiup"]), dtc, N, Hg, Wg, hh, wh, Ck), "resize"),
            ops.Call("srganfd_add_relu", (V(T["theta"]), V(T["phiup"]), V(T["f"]), dtc, N * hh * wh, Ck), "add_relu"),
            b.conv(T["f"], T["sig"], ("f", pre + ".psi"), hh, wh, Ck, 32, cout_store=1, bias=b.P(pre + ".psi.bias"), y_f32=True, **one),
            ops.Call("srganfd_sigmoid", (T["sig"].data_ptr(), T["sig"].numel()), "sigmoid"),
            b.resample(1, T["sig"], T["sigup"], hh, wh, 1, A.F32),
            ops.Call("srganfd_gate_mul", (0, V(B[xname]), T["sigup"].data_ptr(), V(T["y"]), A.NULL_VIEW, None, dtc, N * h * w, Ck), "gate_mul"),
            b.conv(T["y"], T["wy"], ("f", pre + ".W.0"), h, w, Ck, Ck, bias=b.P(pre + ".W.0.bias"), **one),
            sp.bn[k],
        ]

    def _gate_backward(self, sp: _Shape, b: ops.PlanBuilder, k: int, xname: str, dcat, dgated_out, dgated_prev, last: bool) -> list:
        """gate k from the gradient of its half of the concatenation buffer ``dcat``: its shares of B[xname]'s gradient stay in
        D["dxg"] and D["dxt"]; the gating map's gradient goes to ``dgated_out``, ``dgated_prev`` added (``last``: and LeakyReLU' of
        the gating map applied)"""
        N, dtc, nf, B, V = sp.N, sp.dtc, self.nf, sp.B, A.view
        pre, T = f"attn_{k}", sp.attn[k]
        D = T["grad"]
        h, w, hh, wh, Ck = T["dims"]
        Hg, Wg = sp.Rg
        one = dict(ksize=1, pad=0)
        return [
            GateBatchNormBwd(sp.bn[k], V(dcat), V(D["dwy"])),
            b.wgrad(T["y"], D["dwy"], h, w, Ck, Ck, pre + ".W.0.weight", pre + ".W.0.bias", **one),
            b.dgrad(D["dwy"], D["dy"], ("b", pre + ".W.0"), h, w, Ck, Ck, **one),
            ops.Call("srganfd_gate_mul", (1, V(B[xname]), T["sigup"].data_ptr(), V(D["dy"]), V(D["dxg"]), D["dsigup"].data_ptr(), dtc, N * h * w, Ck),
                     "gate_mul_bwd"),
            b.resample(2, D["dsigup"], D["dsig"], hh, wh, 1, A.F32),
            ops.Call("srganfd_sigmoid_bwd", (D["dsig"].data_ptr(), T["sig"].data_ptr(), D["dsig"].data_ptr(), D["dsig"].numel()), "sigmoid_bwd"),
            ops.Call("srganfd_nchw_to_nhwc", (D["dsig"].data_ptr(), N, 1, hh, wh, V(D["dpsip"]), dtc, 32, None, None), "pad32"),
            b.wgrad(T["f"], D["dpsip"], hh, wh, Ck, 32, pre + ".psi.weight", pre + ".psi.bias", cout_real=1, **one),
            b.dgrad(D["dpsip"], D["df"], ("b", pre + ".psi"), hh, wh, 32, Ck, mask=T["f"], mask_slope=0.0, **one),
            b.wgrad(B[xname], D["df"], h, w, Ck, Ck, pre + ".theta.weight", ksize=2, stride=2, pad=0),
            *b.strided_dgrad(D["df"], D["dxt"], ("b", pre + ".theta"), hh, wh, Ck, Ck, 1, 0),      # 2x2 stride 2: four classes of 1x1 convs
            ops.Call("srganfd_resize_bilinear", (1, V(D["df"]), V(D["dphi"]), dtc, N, Hg, Wg, hh, wh, Ck), "resize_bwd"),
            b.wgrad(B["gated"], D["dphi"], Hg, Wg, 4 * nf, Ck, pre + ".phi.weight", pre + ".phi.bias", **one),
            b.dgrad(D["dphi"], dgated_out, ("b", pre + ".phi"), Hg, Wg, Ck, 4 * nf, r1=dgated_prev, mask=B["gated"] if last else None, **one),
        ]

    def _plan_forward(self, sp: _Shape, b: ops.PlanBuilder, train: bool) -> None:
        N, H, W, dtc, nf, V = sp.N, sp.H, sp.W, sp.dtc, self.nf, A.view
        if H % 8 or W % 8:
            raise A.SrganfdError("UNetDiscriminatorAesrgan input height/width must be multiples of 8")
        # conv0 (in_ch -> nf) and conv9 (nf -> 1) on the thin-side kernels in the 16-bit modes (csrc/conv_thin.hip): 4-channel pitch
        sp.thin_i, sp.thin_o = ops.thin_ok(dtc, nf, self.in_ch), ops.thin_ok(dtc, nf, 1)
        self._forward_buffers(sp, b)
        B, R = sp.B, sp.R
        bn_ws = [b.buf(2048 * 256 + 3 * 256, dtype=torch.float32), None]
        sp.bn = {}
        lre = dict(act=A.ACT_LRELU, slope=0.2)
        fw = [
            b.image_to_features(sp.thin_i, B["xin"], B["x0"], "conv0", H, W, self.in_ch, nf, True, **lre),
            b.conv(B["x0"], B["x1"], ("f", "conv1"), *R[0], nf, 2 * nf, stride=2, **lre),
            b.conv(B["x1"], B["x2"], ("f", "conv2"), *R[1], 2 * nf, 4 * nf, stride=2, **lre),
            b.conv(B["x2"], B["x3"], ("f", "conv3"), *R[2], 4 * nf, 8 * nf, stride=2, **lre),
            b.conv(B["x3"], B["gated"], ("f", "gating"), *R[3], 8 * nf, 4 * nf, ksize=1, pad=1, **lre),
        ]
        for k, xname, cat in ((1, "x2", "cat1"), (2, "x1", "cat2"), (3, "x0", "cat3")):
            fw += self._gate_forward(sp, b, k, xname, cat, bn_ws)
        fw += [
            b.resample(1, B["x3"], B["b3"], *R[3], 8 * nf),
            b.conv(B["b3"], V(B["cat1"], c0=4 * nf), ("f", "cat_1.convU"), *R[2], 8 * nf, 4 * nf, **lre),
            b.conv(B["cat1"], B["x4"], ("f", "conv4"), *R[2], 8 * nf, 4 * nf, **lre),
            b.resample(1, B["x4"], B["b4"], *R[2], 4 * nf),
            b.conv(B["b4"], V(B["cat2"], c0=2 * nf), ("f", "cat_2.convU"), *R[1], 4 * nf, 2 * nf, **lre),
            b.conv(B["cat2"], B["x5"], ("f", "conv5"), *R[1], 4 * nf, 2 * nf, **lre),
            b.resample(1, B["x5"], B["b5"], *R[1], 2 * nf),
            b.conv(B["b5"], V(B["cat3"], c0=nf), ("f", "cat_3.convU"), *R[0], 2 * nf, nf, **lre),
            b.conv(B["cat3"], B["x6"], ("f", "conv6"), *R[0], 2 * nf, nf, **lre),
            b.conv(B["x6"], B["c7"], ("f", "conv7"), *R[0], nf, nf, **lre),
            b.conv(B["c7"], B["c8"], ("f", "conv8"), *R[0], nf, nf, **lre),
            # conv9 writes the logits, allocated per forward
            ops.PerCall(b.features_to_image(sp.thin_o, B["c8"], 0, 1, "conv9", H, W, 1, nf, False)),
        ]
        sp.fw = fw

    def _plan_backward(self, sp: _Shape, b: ops.PlanBuilder) -> None:
        N, H, W, nf, V = sp.N, sp.H, sp.W, self.nf, A.view
        self._backward_buffers(sp, b)
        B, G, R = sp.B, sp.G, sp.R
        Hg, Wg = sp.Rg
        P0 = N * H * W
        grad = lambda k, name: sp.attn[k]["grad"][name]

        def sn_wgrad(name, x, dy, h, w, cin, cout, **kw):
            """weight gradient of a spectral-normalised layer: dL/d(W/sigma) goes to the scratch gradient, SnGradBatch finishes the job"""
            return b.wgrad(x, dy, h, w, cin, cout, name + ".weight_orig", sn=SN_INDEX[name], **kw)

        def up_block(k, cat, dcat, bprev, dbprev, dxprev, xprev, conv, dx, h, w, c, npix):
            """conv{4,5,6} over the concatenation buffer ``cat`` and the convU in front of its upper half, down to the LeakyReLU'-masked
            gradient ``dxprev`` of the layer below (``xprev``, half the size; None: the bottom of the U, which the gating conv masks)"""
            out = [sn_wgrad(conv, B[cat], G[dx], h, w, 2 * c, c),
                   b.dgrad(G[dx], G[dcat], ("b", conv), h, w, c, 2 * c),
                   b.lrelu_bwd(V(G[dcat], c0=c), V(B[cat], c0=c), V(G[dcat], c0=c), npix, c),
                   sn_wgrad(f"cat_{k}.convU", B[bprev], V(G[dcat], c0=c), h, w, 2 * c, c),
                   b.dgrad(V(G[dcat], c0=c), G[dbprev], ("b", f"cat_{k}.convU"), h, w, c, 2 * c),
                   b.resample(2, G[dbprev], G[dxprev], h // 2, w // 2, 2 * c)]
            if xprev is not None:
                out.append(b.lrelu_bwd(G[dxprev], B[xprev], G[dxprev], npix // 4, 2 * c))
            return out
        bw = [
            b.image_wgrad(sp.thin_o, sp.dl, B["c8"], "conv9", sp.thin_ws, H, W, 1, nf, False),
            b.image_to_features(sp.thin_o, sp.dl, G["g8"], "conv9", H, W, 1, nf, False, flip=True, mask=V(B["c8"]), mask_slope=0.2),
            sn_wgrad("conv8", B["c7"], G["g8"], H, W, nf, nf),
            b.dgrad(G["g8"], G["g7"], ("b", "conv8"), H, W, nf, nf, mask=B["c7"]),
            sn_wgrad("conv7", B["x6"], G["g7"], H, W, nf, nf),
            b.dgrad(G["g7"], G["g6"], ("b", "conv7"), H, W, nf, nf, mask=B["x6"]),
        ]
        bw += up_block(3, "cat3", "dc3", "b5", "db5", "dx5", "x5", "conv6", "g6", *R[0], nf, P0)
        bw += self._gate_backward(sp, b, 3, "x0", G["dc3"], G["dgated"][0], None, False)
        bw += up_block(2, "cat2", "dc2", "b4", "db4", "dx4", "x4", "conv5", "dx5", *R[1], 2 * nf, P0 // 4)
        bw += self._gate_backward(sp, b, 2, "x1", G["dc2"], G["dgated"][1], G["dgated"][0], False)
        bw += up_block(1, "cat1", "dc1", "b3", "db3", "dx3a", None, "conv4", "dx4", *R[2], 4 * nf, P0 // 16)
        bw += self._gate_backward(sp, b, 1, "x2", G["dc1"], G["dgated"][2], G["dgated"][1], True)
        dgated = G["dgated"][2]      # sum of the three gates' gradients, LeakyReLU' of `gated` applied
        bw += [
            sn_wgrad("gating", B["x3"], dgated, *R[3], 8 * nf, 4 * nf, ksize=1, pad=1),
            b.dgrad(dgated, G["dx3"], ("b", "gating"), Hg, Wg, 4 * nf, 8 * nf, r1=G["dx3a"], mask=B["x3"], ksize=1, pad=-1),
            sn_wgrad("conv3", B["x2"], G["dx3"], *R[2], 4 * nf, 8 * nf, stride=2),
            # the 3x3 stride-2 data gradients: 4 parity classes of 2x2-tap convs, each with its gate's two shares of the skip's gradient
            *b.strided_dgrad(G["dx3"], G["dx2"], ("b", "conv3"), *R[3], 8 * nf, 4 * nf, 2, 0, r1=grad(1, "dxg"), r2=grad(1, "dxt"), mask=B["x2"]),
            sn_wgrad("conv2", B["x1"], G["dx2"], *R[1], 2 * nf, 4 * nf, stride=2),
            *b.strided_dgrad(G["dx2"], G["dx1"], ("b", "conv2"), *R[2], 4 * nf, 2 * nf, 2, 0, r1=grad(2, "dxg"), r2=grad(2, "dxt"), mask=B["x1"]),
            sn_wgrad("conv1", B["x0"], G["dx1"], *R[0], nf, 2 * nf, stride=2),
            *b.strided_dgrad(G["dx1"], G["dx0"], ("b", "conv1"), *R[1], 2 * nf, nf, 2, 0, r1=grad(3, "dxg"), r2=grad(3, "dxt"), mask=B["x0"]),
            b.image_wgrad(sp.thin_i, B["xin"], G["dx0"], "conv0", sp.thin_ws, H, W, self.in_ch, nf, True),
        ]
        sp.dx_conv = first_layer_dgrad(b.features_to_image(sp.thin_i, G["dx0"], sp.dxp, 4, "conv0", H, W, self.in_ch, nf, True, flip=True))
        sp.bw = bw
        self._backward_workspaces(sp, b)

    # ---- execution: EngineBase's passes; the attention maps of the last forward are kept on the module ----
    def forward(self, x: Tensor, training: bool) -> Tensor:
        logits = super().forward(x, training)
        sp, o = self._last, self.owner
        o.ly1, o.ly2, o.ly3 = (sp.attn[k]["sigup"].view(sp.N, 1, *sp.attn[k]["dims"][:2]).clone() for k in (1, 2, 3))
        return logits


def aesrgan_engine(owner: nn.Module) -> AesrganDiscriminatorEngine:
    return _engine(owner, lambda: AesrganDiscriminatorEngine(owner))


def aesrgan_discriminator_apply(owner: nn.Module, x: Tensor) -> Tensor:
    return engine_apply(aesrgan_engine(owner), x, owner.training)
