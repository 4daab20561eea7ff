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

    # ---- plan ----
    def _plan(self, N, H, W, dt, dtc, device, pk, train=True):
        key = (N, H, W, dtc, str(device), pk["buf"].data_ptr(), self.fp.flat.data_ptr())
        sp = self.shapes.get(key)
        if sp is not None:
            return sp
        if H % 8 or W % 8:
            raise A.SrganfdError("UNetDiscriminatorAesrgan input height/width must be multiples of 8")
        sp = _Shape()
        sp.N, sp.H, sp.W, sp.dt, sp.dtc, sp.device = N, H, W, dt, dtc, device
        V = A.view
        fptr, wptr, O = self.fp.flat.data_ptr(), pk["buf"].data_ptr(), pk["offs"]
        P = lambda name: fptr + 4 * self._poff(name)      # (used while the plan is built only, not stored on it)
        Wp = lambda *key: wptr + O[key]
        nf = self.nf

        def new(h, w, c, dtype=dt):
            return torch.empty(N, h, w, c, dtype=dtype, device=device)
        R = [(H >> k, W >> k) for k in range(4)]
        Hg, Wg = R[3][0] + 2, R[3][1] + 2
        B = sp.B = {}
        # conv0 (in_ch -> nf) and conv9 (nf -> 1) on the thin-side kernels in the 16-bit modes (csrc/conv_thin.hip): 4-channel pitch
        sp.thin_i, sp.thin_o = ops.thin_ok(dtc, nf, self.in_ch), ops.thin_ok(dtc, nf, 1)
        B["xin"] = sp.xin = new(H, W, 4 if sp.thin_i else 32)
        B["x0"], B["x1"], B["x2"], B["x3"] = new(*R[0], nf), new(*R[1], 2 * nf), new(*R[2], 4 * nf), new(*R[3], 8 * nf)
        B["gated"] = new(Hg, Wg, 4 * nf)
        B["cat1"], B["cat2"], B["cat3"] = new(*R[2], 8 * nf), new(*R[1], 4 * nf), new(*R[0], 2 * nf)
        B["b3"], B["x4"], B["b4"], B["x5"], B["b5"] = new(*R[2], 8 * nf), new(*R[2], 4 * nf), new(*R[1], 4 * nf), new(*R[1], 2 * nf), new(*R[0], 2 * nf)
        B["x6"], B["c7"], B["c8"] = new(*R[0], nf), new(*R[0], nf), new(*R[0], nf)
        bn_ws = [torch.empty(2048 * 256 + 3 * 256, dtype=torch.float32, device=device), None]
        sp.bn = {}
        lre = dict(act=A.ACT_LRELU, slope=0.2)
        cv = lambda *a, **k: ops.Conv(ops.conv_args(dtc, *a, **k))
        rs = lambda op, a, b, h, w, c, dtype=dtc: ops.Call("srganfd_resample", (op, a, b, dtype, N, h, w, c), "resample")
        fw = [
            ops.image_to_features(dtc, sp.thin_i, B["xin"], V(B["x0"]), P("conv0.weight"), Wp("f", "conv0"), N, H, W, self.in_ch, nf, True,
                                  bias=P("conv0.bias"), **lre),
            cv(V(B["x0"]), V(B["x1"]), Wp("f", "conv1"), N, *R[0], nf, 2 * nf, stride=2, **lre),
            cv(V(B["x1"]), V(B["x2"]), Wp("f", "conv2"), N, *R[1], 2 * nf, 4 * nf, stride=2, **lre),
            cv(V(B["x2"]), V(B["x3"]), Wp("f", "conv3"), N, *R[2], 4 * nf, 8 * nf, stride=2, **lre),
            cv(V(B["x3"]), V(B["gated"]), Wp("f", "gating"), N, *R[3], 8 * nf, 4 * nf, ksize=1, pad=1, **lre),
        ]
        sp.attn = {}
        for k, xname, cat in ((1, "x2", "cat1"), (2, "x1", "cat2"), (3, "x0", "cat3")):
            pre = f"attn_{k}"
            Ck = B[xname].shape[-1]
            h, w = R[3 - k]
            hh, wh = h // 2, w // 2
            T = {}
            T["theta"], T["phi"], T["phiup"], T["f"] = new(hh, wh, Ck), new(Hg, Wg, Ck), new(hh, wh, Ck), new(hh, wh, Ck)
            T["sig"] = torch.empty(N, hh, wh, 1, dtype=torch.float32, device=device)
            T["sigup"] = torch.empty(N, h, w, 1, dtype=torch.float32, device=device)
            T["y"], T["wy"] = new(h, w, Ck), new(h, w, Ck)
            T["save"] = torch.empty(4 * Ck, dtype=torch.float32, device=device)
            T["dims"] = (h, w, hh, wh, Ck)
            sp.attn[k] = T
            fw += [
                cv(V(B[xname]), V(T["theta"]), Wp("f", pre + ".theta"), N, h, w, Ck, Ck, ksize=2, stride=2, pad=0),
                cv(V(B["gated"]), V(T["phi"]), Wp("f", pre + ".phi"), N, Hg, Wg, 4 * nf, Ck, ksize=1, pad=0, bias=P(pre + ".phi.bias")),
                ops.Call("srganfd_resize_bilinear", (0, V(T["phi"]), V(T["phiup"]), dtc, N, Hg, Wg, hh, wh, Ck), "resize"),
                ops.Call("srganfd_add_relu", (V(T["theta"]), V(T["phiup"]), V(T["f"]), dtc, N * hh * wh, Ck), "add_relu"),
                cv(V(T["f"]), V(T["sig"]), Wp("f", pre + ".psi"), N, hh, wh, Ck, 32, ksize=1, pad=0, cout_store=1, bias=P(pre + ".psi.bias"), y_f32=True),
                ops.Call("srganfd_sigmoid", (T["sig"].data_ptr(), T["sig"].numel()), "sigmoid"),
                rs(1, V(T["sig"]), V(T["sigup"]), hh, wh, 1, A.F32),
                ops.Call("srganfd_gate_mul", (0, V(B[xname]), T["sigup"].data_ptr(), V(T["y"]), A.NULL_VIEW, None, dtc, N * h * w, Ck), "gate_mul"),
                cv(V(T["y"]), V(T["wy"]), Wp("f", pre + ".W.0"), N, h, w, Ck, Ck, ksize=1, pad=0, bias=P(pre + ".W.0.bias")),
            ]
            sp.bn[k] = GateBatchNorm(self, V(T["wy"]), V(B[cat]), dtc, N * h * w, Ck, self._poff(pre + ".W.1.weight"), self._poff(pre + ".W.1.bias"),
                                     _mod(self.owner, pre + ".W.1"), T["save"], bn_ws)
            fw.append(sp.bn[k])
        fw += [
            rs(1, V(B["x3"]), V(B["b3"]), *R[3], 8 * nf),
            cv(V(B["b3"]), V(B["cat1"], c0=4 * nf), Wp("f", "cat_1.convU"), N, *R[2], 8 * nf, 4 * nf, **lre),
            cv(V(B["cat1"]), V(B["x4"]), Wp("f", "conv4"), N, *R[2], 8 * nf, 4 * nf, **lre),
            rs(1, V(B["x4"]), V(B["b4"]), *R[2], 4 * nf),
            cv(V(B["b4"]), V(B["cat2"], c0=2 * nf), Wp("f", "cat_2.convU"), N, *R[1], 4 * nf, 2 * nf, **lre),
            cv(V(B["cat2"]), V(B["x5"]), Wp("f", "conv5"), N, *R[1], 4 * nf, 2 * nf, **lre),
            rs(1, V(B["x5"]), V(B["b5"]), *R[1], 2 * nf),
            cv(V(B["b5"]), V(B["cat3"], c0=nf), Wp("f", "cat_3.convU"), N, *R[0], 2 * nf, nf, **lre),
            cv(V(B["cat3"]), V(B["x6"]), Wp("f", "conv6"), N, *R[0], 2 * nf, nf, **lre),
            cv(V(B["x6"]), V(B["c7"]), Wp("f", "conv7"), N, *R[0], nf, nf, **lre),
            cv(V(B["c7"]), V(B["c8"]), Wp("f", "conv8"), N, *R[0], nf, nf, **lre),
        ]
        # conv9 writes the logits, allocated per forward
        fw.append(ops.PerCall(ops.features_to_image(dtc, sp.thin_o, V(B["c8"]), 0, 1, P("conv9.weight"), Wp("f", "conv9"), N, H, W, 1, nf, False,
                                                    bias=P("conv9.bias"))))
        sp.fw = fw
        sp.R, sp.Rg = R, (Hg, Wg)
        self._plan_backward(sp, pk)
        self.shapes[key] = sp
        return sp

    def _plan_backward(self, sp, pk):
        N, H, W, dt, dtc, device = sp.N, sp.H, sp.W, sp.dt, sp.dtc, sp.device
        V, B, R, nf = A.view, sp.B, sp.R, self.nf
        Hg, Wg = sp.Rg
        wptr, O = pk["buf"].data_ptr(), pk["offs"]
        Wp = lambda *key: wptr + O[key]
        fptr = self.fp.flat.data_ptr()
        P = lambda name: fptr + 4 * self.fp.off(name)      # (used while the plan is built only, not stored on it)

        def new(h, w, c, dtype=dt):
            return torch.empty(N, h, w, c, dtype=dtype, device=device)
        wplans = ops.WgradPlans(device, dtc, N)

        def wg(name, x, dy, h, w, cin, cout, k=3, s=1, pad=1, sn=False, cin_real=None, cout_real=None, bias=False, dy_c0=0):
            plan = wplans.conv(h, w, cin, cout, self._poff(name + (".weight_orig" if sn else ".weight")), self._poff(name + ".bias") if bias else -1,
                               cin_real, cout_real, ksize=k, stride=s, pad=pad)
            return ops.Wgrad(plan, V(x), V(dy, c0=dy_c0), sn=SN_INDEX[name] if sn else None)

        cv = lambda *a, **k: ops.Conv(ops.conv_args(dtc, *a, **k))
        rs = lambda op, a, b, h, w, c, dtype=dtc: ops.Call("srganfd_resample", (op, a, b, dtype, N, h, w, c), "resample")
        lb = lambda dy, act, out, npix, c, slope=0.2: ops.Call("srganfd_lrelu_bwd", (dy, act, A.NULL_VIEW, out, dtc, npix, c, slope), "lrelu_bwd")

        def strided_dgrad(key, ks, dy, dx, hd, wd, cin_op, cout_op, r1=None, r2=None, mask=None):
            """4 parity classes writing a (2hd x 2wd) image: ks=2 (3x3 s2 conv) or ks=1 (2x2 s2 conv)"""
            view = lambda t: None if t is None else V(t)
            return ops.parity_class_launches(      # class_pad 0: every class reads the same window of dy
                dtc, V(dy), V(dx), wptr, [O[key + (c,)] for c in range(4)], N, hd, wd, cin_op, cout_op, ks, 0,
                **ops.dgrad_epilogue(view(r1), view(r2), view(mask)))

        sp.dl = new(H, W, 4 if sp.thin_o else 32)
        sp.thin_ws = torch.empty(ops.thin_wgrad_workspace_bytes(), dtype=torch.uint8, device=device) if (sp.thin_i or sp.thin_o) else None
        G = sp.G = {}
        G["g8"], G["g7"], G["g6"] = new(*R[0], nf), new(*R[0], nf), new(*R[0], nf)
        G["dc3"], G["db5"], G["dx5"] = new(*R[0], 2 * nf), new(*R[0], 2 * nf), new(*R[1], 2 * nf)
        G["dc2"], G["db4"], G["dx4"] = new(*R[1], 4 * nf), new(*R[1], 4 * nf), new(*R[2], 4 * nf)
        G["dc1"], G["db3"], G["dx3a"], G["dx3"] = new(*R[2], 8 * nf), new(*R[2], 8 * nf), new(*R[3], 8 * nf), new(*R[3], 8 * nf)
        G["dx2"], G["dx1"], G["dx0"] = new(*R[2], 4 * nf), new(*R[1], 2 * nf), new(*R[0], nf)
        G["dgated"] = [new(Hg, Wg, 4 * nf) for _ in range(3)]
        sp.dxp = new(H, W, 4, dtype=torch.float32)
        P0 = N * H * W

        def attn_bwd(k, xname, dcat, dgated_out, dgated_prev, last):
            pre = f"attn_{k}"
            T = sp.attn[k]
            h, w, hh, wh, Ck = T["dims"]
            D = T["grad"] = {}
            D["dwy"], D["dy"], D["dxg"] = new(h, w, Ck), new(h, w, Ck), new(h, w, Ck)
            D["dsigup"] = torch.empty(N, h, w, 1, dtype=torch.float32, device=device)
            D["dsig"] = torch.empty(N, hh, wh, 1, dtype=torch.float32, device=device)
            D["dpsip"], D["df"], D["dxt"], D["dphi"] = new(hh, wh, 32), new(hh, wh, Ck), new(h, w, Ck), new(Hg, Wg, Ck)
            items = [
                GateBatchNormBwd(sp.bn[k], V(dcat), V(D["dwy"])),
                wg(pre + ".W.0", T["y"], D["dwy"], h, w, Ck, Ck, k=1, pad=0, bias=True),
                cv(V(D["dwy"]), V(D["dy"]), Wp("b", pre + ".W.0"), N, h, w, Ck, Ck, ksize=1, pad=0),
                ops.Call("srganfd_gate_mul", (1, V(B[xname]), T["sigup"].data_ptr(), V(D["dy"]), V(D["dxg"]), D["dsigup"].data_ptr(), dtc, N * h * w, Ck),
                         "gate_mul_bwd"),
                rs(2, V(D["dsigup"]), V(D["dsig"]), hh, wh, 1, A.F32),
                ops.Call("srganfd_sigmoid_bwd", (D["dsig"].data_ptr(), T["sig"].data_ptr(), D["dsig"].data_ptr(), D["dsig"].numel()), "sigmoid_bwd"),
                ops.Call("srganfd_nchw_to_nhwc", (D["dsig"].data_ptr(), N, 1, hh, wh, V(D["dpsip"]), dtc, 32, None, None), "pad32"),
                wg(pre + ".psi", T["f"], D["dpsip"], hh, wh, Ck, 32, k=1, pad=0, cout_real=1, bias=True),
                cv(V(D["dpsip"]), V(D["df"]), Wp("b", pre + ".psi"), N, hh, wh, 32, Ck, ksize=1, pad=0, mask=V(T["f"]), mask_slope=0.0),
                wg(pre + ".theta", B[xname], D["df"], h, w, Ck, Ck, k=2, s=2, pad=0),
            ]
            items += strided_dgrad(("b", pre + ".theta"), 1, D["df"], D["dxt"], hh, wh, Ck, Ck)
            items += [
                ops.Call("srganfd_resize_bilinear", (1, V(D["df"]), V(D["dphi"]), dtc, N, Hg, Wg, hh, wh, Ck), "resize_bwd"),
                wg(pre + ".phi", B["gated"], D["dphi"], Hg, Wg, 4 * nf, Ck, k=1, pad=0, bias=True),
                cv(V(D["dphi"]), V(dgated_out), Wp("b", pre + ".phi"), N, Hg, Wg, Ck, 4 * nf, ksize=1, pad=0,
                   r1=V(dgated_prev) if dgated_prev is not None else A.NULL_VIEW, r1_scale=1.0 if dgated_prev is not None else 0.0,
                   mask=V(B["gated"]) if last else A.NULL_VIEW, mask_slope=0.2),
            ]
            return items

        bw = [
            ops.image_wgrad(dtc, sp.thin_o, wplans, sp.dl, B["c8"], P("conv9.weight"), self._poff("conv9.weight"), self._poff("conv9.bias"), sp.thin_ws,
                            N, H, W, 1, nf, False),
            ops.image_to_features(dtc, sp.thin_o, sp.dl, V(G["g8"]), P("conv9.weight"), Wp("b", "conv9"), N, H, W, 1, nf, False, flip=True,
                                  mask=V(B["c8"]), mask_slope=0.2),
            wg("conv8", B["c7"], G["g8"], H, W, nf, nf, sn=True),
            cv(V(G["g8"]), V(G["g7"]), Wp("b", "conv8"), N, H, W, nf, nf, mask=V(B["c7"]), mask_slope=0.2),
            wg("conv7", B["x6"], G["g7"], H, W, nf, nf, sn=True),
            cv(V(G["g7"]), V(G["g6"]), Wp("b", "conv7"), N, H, W, nf, nf, mask=V(B["x6"]), mask_slope=0.2),
            wg("conv6", B["cat3"], G["g6"], H, W, 2 * nf, nf, sn=True),
            cv(V(G["g6"]), V(G["dc3"]), Wp("b", "conv6"), N, H, W, nf, 2 * nf),
            lb(V(G["dc3"], c0=nf), V(B["cat3"], c0=nf), V(G["dc3"], c0=nf), P0, nf),
            wg("cat_3.convU", B["b5"], G["dc3"], H, W, 2 * nf, nf, sn=True, dy_c0=nf),
            cv(V(G["dc3"], c0=nf), V(G["db5"]), Wp("b", "cat_3.convU"), N, H, W, nf, 2 * nf),
            rs(2, V(G["db5"]), V(G["dx5"]), *R[1], 2 * nf),
            lb(V(G["dx5"]), V(B["x5"]), V(G["dx5"]), P0 // 4, 2 * nf),
        ]
        bw += attn_bwd(3, "x0", G["dc3"], G["dgated"][0], None, False)
        bw += [
            wg("conv5", B["cat2"], G["dx5"], *R[1], 4 * nf, 2 * nf, sn=True),
            cv(V(G["dx5"]), V(G["dc2"]), Wp("b", "conv5"), N, *R[1], 2 * nf, 4 * nf),
            lb(V(G["dc2"], c0=2 * nf), V(B["cat2"], c0=2 * nf), V(G["dc2"], c0=2 * nf), P0 // 4, 2 * nf),
            wg("cat_2.convU", B["b4"], G["dc2"], *R[1], 4 * nf, 2 * nf, sn=True, dy_c0=2 * nf),
            cv(V(G["dc2"], c0=2 * nf), V(G["db4"]), Wp("b", "cat_2.convU"), N, *R[1], 2 * nf, 4 * nf),
            rs(2, V(G["db4"]), V(G["dx4"]), *R[2], 4 * nf),
            lb(V(G["dx4"]), V(B["x4"]), V(G["dx4"]), P0 // 16, 4 * nf),
        ]
        bw += attn_bwd(2, "x1", G["dc2"], G["dgated"][1], G["dgated"][0], False)
        bw += [
            wg("conv4", B["cat1"], G["dx4"], *R[2], 8 * nf, 4 * nf, sn=True),
            cv(V(G["dx4"]), V(G["dc1"]), Wp("b", "conv4"), N, *R[2], 4 * nf, 8 * nf),
            lb(V(G["dc1"], c0=4 * nf), V(B["cat1"], c0=4 * nf), V(G["dc1"], c0=4 * nf), P0 // 16, 4 * nf),
            wg("cat_1.convU", B["b3"], G["dc1"], *R[2], 8 * nf, 4 * nf, sn=True, dy_c0=4 * nf),
            cv(V(G["dc1"], c0=4 * nf), V(G["db3"]), Wp("b", "cat_1.convU"), N, *R[2], 4 * nf, 8 * nf),
            rs(2, V(G["db3"]), V(G["dx3a"]), *R[3], 8 * nf),
        ]
        bw += attn_bwd(1, "x2", G["dc1"], G["dgated"][2], G["dgated"][1], True)
        dgated = G["dgated"][2]      # sum of the three gates' gradients, LeakyReLU' of `gated` applied
        bw += [
            wg("gating", B["x3"], dgated, *R[3], 8 * nf, 4 * nf, k=1, pad=1, sn=True),
            cv(V(dgated), V(G["dx3"]), Wp("b", "gating"), N, Hg, Wg, 4 * nf, 8 * nf, ksize=1, pad=-1, r1=V(G["dx3a"]), r1_scale=1.0,
               mask=V(B["x3"]), mask_slope=0.2),
            wg("conv3", B["x2"], G["dx3"], *R[2], 4 * nf, 8 * nf, s=2, sn=True),
        ]
        bw += strided_dgrad(("b", "conv3"), 2, G["dx3"], G["dx2"], *R[3], 8 * nf, 4 * nf,
                            r1=sp.attn[1]["grad"]["dxg"], r2=sp.attn[1]["grad"]["dxt"], mask=B["x2"])
        bw.append(wg("conv2", B["x1"], G["dx2"], *R[1], 2 * nf, 4 * nf, s=2, sn=True))
        bw += strided_dgrad(("b", "conv2"), 2, G["dx2"], G["dx1"], *R[2], 4 * nf, 2 * nf,
                            r1=sp.attn[2]["grad"]["dxg"], r2=sp.attn[2]["grad"]["dxt"], mask=B["x1"])
        bw.append(wg("conv1", B["x0"], G["dx1"], *R[0], nf, 2 * nf, s=2, sn=True))
        bw += strided_dgrad(("b", "conv1"), 2, G["dx1"], G["dx0"], *R[1], 2 * nf, nf,
                            r1=sp.attn[3]["grad"]["dxg"], r2=sp.attn[3]["grad"]["dxt"], mask=B["x0"])
        bw.append(ops.image_wgrad(dtc, sp.thin_i, wplans, B["xin"], G["dx0"], P("conv0.weight"), self._poff("conv0.weight"), self._poff("conv0.bias"),
                                  sp.thin_ws, N, H, W, self.in_ch, nf, True))
        sp.dx_conv = first_layer_dgrad(ops.features_to_image(dtc, sp.thin_i, V(G["dx0"]), sp.dxp, 4, P("conv0.weight"), Wp("b", "conv0"), N, H, W,
                                                             self.in_ch, nf, True, flip=True))
        sp.bw = bw
        self._backward_workspaces(sp, wplans, pk)

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
