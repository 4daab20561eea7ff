"""The two VGG-19 content losses: BSRGAN's five-node, forward-only one (ContentLossEngine) and ESRGAN's differentiable single-node
one (ContentLossGradEngine).  Both run SR and GT through the extractor as one 2N batch of normalised NHWC images, pack
``features.*`` the same way and put ``features.0`` (3 -> 64) on the thin-side kernel in the 16-bit modes (VggEngineBase).

ContentLossEngine: ContentLoss.forward BSRGAN/model.py:536-554 (the reference detaches the result, :552).

ContentLossGradEngine: ESRGAN/model.py:258-292.  ESRGAN's ContentLoss is ``F.l1_loss(vgg(sr)[node], vgg(gt)[node])`` with ONE node (``features.34`` in esrgan_config) and,
unlike BSRGAN's five-node version, it stays in the autograd graph: the generator receives its gradient, so the frozen
VGG needs a backward pass.  SR and GT run through the extractor as one 2N batch; every ReLU output of the SR half is kept.
Backward = sign(sr_f - gt_f) / numel at the node, then per conv the data-gradient launch of the implicit-GEMM kernel with
the previous ReLU's mask in its epilogue, max-pool backward fused with the ReLU derivative in front of the pool, and the
final relayout that undoes the normalisation's 1/std.  No weight gradients (the extractor is frozen, model.py:275-277).
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor, nn

from . import _abi as A
from . import ops
from .engine import EngineBase, _dt, _engine, _require_gpu, _Shape


class VggEngineBase(EngineBase):
    """the convs of ``owner.features[:layers]`` as one flat parameter buffer, packed for the forward pass and, with ``dgrad``, for the
    data gradient; the 2N-batch input; the launch of one feature conv"""
    dgrad = False
    always_backward = True             # (one plan per shape: the differentiable loss's with its backward list, the other's without)

    def __init__(self, owner: nn.Module, layers: int):
        self.convs = [(i, m) for i, m in enumerate(owner.features[:layers]) if isinstance(m, nn.Conv2d)]
        super().__init__(owner, [(f"features.{i}.{k}", getattr(m, k)) for i, m in self.convs for k in ("weight", "bias")])
        self.in_ch = self.convs[0][1].weight.shape[1]

    def _fkey(self, i: int):
        """key of features.i's forward operand in the pack record (the forward-only engine has no other operands)"""
        return ("f", i) if self.dgrad else i

    def _build_pack(self, dtc: int, device) -> dict:
        pb = ops.PackBuilder(dtc)
        for i, m in self.convs:
            co, ci = m.weight.shape[:2]
            pb.fwd(self._fkey(i), self._poff(f"features.{i}.weight"), co, ci)
            if self.dgrad:
                pb.bwd(("b", i), self._poff(f"features.{i}.weight"), co, ci)
        return pb.finish(device)

    def _new_input(self, sp: _Shape, b: ops.PlanBuilder) -> None:
        # features.0 (3 -> 64) on the thin-side kernels in the 16-bit modes (csrc/conv_thin.hip): the normalised image is NHWC with a
        # 4-channel pitch
        sp.thin = ops.thin_ok(sp.dtc, self.owner.features[0].weight.shape[0], self.in_ch)
        sp.xin = b.buf(2 * sp.N, sp.H, sp.W, 4 if sp.thin else 32)

    def _plan_backward(self, sp: _Shape, b: ops.PlanBuilder) -> None:
        """(the forward-only loss has none)"""

    def _load_input(self, sp: _Shape, sr: Tensor, gt: Tensor, dtc: int, L, st) -> None:
        """SR into the first N images of sp.xin, GT into the other N, normalised with the module's mean / std"""
        N, cin, H, W = sr.shape
        mean, std = self.owner.mean, self.owner.std
        cpad = sp.xin.shape[-1]
        for img, half in ((sr, 0), (gt, 1)):
            img = img.detach().contiguous().float()
            dst = A.View(sp.xin.data_ptr() + half * N * H * W * cpad * sp.xin.element_size(), cpad, 0)
            A.check(L.srganfd_nchw_to_nhwc(img.data_ptr(), N, cin, H, W, dst, dtc, cpad, mean.data_ptr(), std.data_ptr(), st), "nchw_to_nhwc")

    def _feature_conv(self, sp: _Shape, b: ops.PlanBuilder, idx: int, x: Tensor, y: Tensor, cin: int, act: int):
        """launch item (ops.Conv or ops.ThinLaunch) of features.idx + activation over the 2N batch: x (its padded channel count is cin) -> y"""
        n, h, w, co = y.shape
        bias = b.P(f"features.{idx}.bias")
        if idx == 0 and sp.thin:
            return ops.ThinLaunch("thin_in", ops.thin_args(b.dtc, n, h, w, self.in_ch, b.P("features.0.weight"), A.view(y), w_big_is_cout=True, bias=bias,
                                                           act=act, thin=sp.xin))
        return ops.Conv(ops.conv_args(b.dtc, A.view(x), A.view(y), b.Wp(self._fkey(idx)), n, h, w, cin, co, bias=bias, act=act))


class LossTap:
    """L1 distance between the SR half ``a`` and the GT half ``b`` of a feature map (``npix`` pixels of ``channels``), written to float
    ``slot`` of the pass's loss vector (``run.out``, zeroed per call)"""
    kind = "loss_tap"

    def __init__(self, feat: Tensor, dtc: int, slot: int, ws: Tensor):
        n2, h, w, c = feat.shape
        gt_half = feat.data_ptr() + feat[:n2 // 2].numel() * feat.element_size()
        self.a, self.b = A.View(feat.data_ptr(), c, 0), A.View(gt_half, c, 0)
        self.dtc, self.npix, self.channels, self.slot, self.ws = dtc, n2 // 2 * h * w, c, slot, ws

    def launch(self, run: ops.Run) -> None:
        A.check(run.L.srganfd_l1_loss_views(self.a, self.b, self.dtc, self.npix, self.channels, 0, 1.0, run.out + 4 * self.slot, 0, self.ws.data_ptr(),
                                            run.st), "l1_views")


class ContentLossEngine(VggEngineBase):
    def __init__(self, owner: nn.Module):
        super().__init__(owner, len(owner.features))
        self.want = [int(n.split(".")[1]) for n in owner.feature_model_extractor_nodes]

    def _plan_forward(self, sp: _Shape, b: ops.PlanBuilder, train: bool) -> None:
        N, dtc = sp.N, sp.dtc
        self._new_input(sp, b)
        sp.bufs = {}
        sp.ws = b.buf(A.LOSS_WS_FLOATS, dtype=torch.float32)
        last = max(self.want)
        post = self.owner.taps_post_relu
        cur, ch, h, w = sp.xin, 32, sp.H, sp.W

        def buf(tag, hh, ww, cc):
            """the feature maps alternate between two buffers per size (``tag`` 0 / 1), the pooled ones have their own ("p")"""
            if (tag, hh, ww, cc) not in sp.bufs:
                sp.bufs[(tag, hh, ww, cc)] = b.buf(2 * N, hh, ww, cc)
            return sp.bufs[(tag, hh, ww, cc)]
        fw, flip = [], 0
        for idx in range(last + 1):
            m = self.owner.features[idx]
            if isinstance(m, nn.Conv2d):
                co = m.weight.shape[0]
                out = buf(flip, h, w, co)
                flip ^= 1
                tap = idx in self.want
                # taps are observed after the in-place ReLU unless they are the last requested node
                relu_in_conv = not (tap and (idx == last or not post))
                fw.append(self._feature_conv(sp, b, idx, cur, out, ch, A.ACT_RELU if relu_in_conv else A.ACT_NONE))
                if tap:
                    fw.append(LossTap(out, dtc, self.want.index(idx), sp.ws))
                    if not relu_in_conv and idx != last:
                        fw.append(b.resample(4, out, out, h, w, co, n=2 * N, what="relu"))
                cur, ch = out, co
            elif isinstance(m, nn.MaxPool2d):
                out = buf("p", h // 2, w // 2, ch)
                fw.append(b.resample(3, cur, out, h, w, ch, n=2 * N, what="maxpool"))
                cur, h, w = out, h // 2, w // 2
        sp.fw = fw

    def forward(self, sr: Tensor, gt: Tensor) -> Tensor:
        _require_gpu(sr)
        dt, dtc = _dt(self.owner)
        dev = sr.device
        pk = self._ensure_packed(dtc, dev)
        N, Cin, H, W = sr.shape
        if H < 16 or W < 16:
            raise A.SrganfdError("ContentLoss input height/width must be at least 16 (four 2x2 max-pools; odd sizes floor like torch)")
        L, st = A.lib(), A.stream_ptr()
        sp = self._last = self._plan(N, H, W, dt, dtc, dev, pk, True)
        self._load_input(sp, sr, gt, dtc, L, st)
        losses = torch.zeros(len(self.want), dtype=torch.float32, device=dev)
        ops.run_items(sp.fw, ops.Run("conv2d(vgg)", out=losses.data_ptr()))
        return losses.view(1, -1)


def content_loss_apply(owner: nn.Module, sr: Tensor, gt: Tensor) -> Tensor:
    eng = _engine(owner, lambda: ContentLossEngine(owner))
    with torch.no_grad():
        return eng.forward(sr, gt)


class ContentLossGradEngine(VggEngineBase):
    dgrad = True

    def __init__(self, owner: nn.Module):
        self.last = int(owner.feature_model_extractor_nodes[0].split(".")[1])
        if not isinstance(owner.features[self.last], nn.Conv2d):
            raise A.SrganfdError("differentiable ContentLoss: the node must be a conv of vgg19.features (esrgan_config uses features.34)")
        super().__init__(owner, self.last + 1)

    def _plan_forward(self, sp: _Shape, b: ops.PlanBuilder, train: bool) -> None:
        N, H, W, dtc = sp.N, sp.H, sp.W, sp.dtc
        self._new_input(sp, b)      # (thin: features.0's data gradient runs on the thin-side kernel too)
        fw, chain = [], []          # chain: (layer, index, input, output, h, w, cin, cout) in forward order
        cur, ch, h, w = sp.xin, 32, H, W
        sp.keep = [sp.xin]
        for idx in range(self.last + 1):
            m = self.owner.features[idx]
            if isinstance(m, nn.Conv2d):
                co = m.weight.shape[0]
                out = b.buf(2 * N, h, w, co)
                fw.append(self._feature_conv(sp, b, idx, cur, out, ch, A.ACT_NONE if idx == self.last else A.ACT_RELU))
                chain.append(("conv", idx, cur, out, h, w, ch, co))
                cur, ch = out, co
            elif isinstance(m, nn.MaxPool2d):
                out = b.buf(2 * N, h // 2, w // 2, ch)
                fw.append(b.resample(3, cur, out, h, w, ch, n=2 * N, what="maxpool"))
                chain.append(("pool", idx, cur, out, h, w, ch, ch))
                cur, h, w = out, h // 2, w // 2
            sp.keep.append(cur)
        sp.feat, sp.feat_dims, sp.chain = cur, (h, w, ch), chain
        sp.ws = b.buf(A.LOSS_WS_FLOATS, dtype=torch.float32)
        fw.append(LossTap(cur, dtc, 0, sp.ws))           # the loss, a one-element vector allocated per forward
        sp.fw = fw

    def _plan_backward(self, sp: _Shape, b: ops.PlanBuilder) -> None:
        """the SR half only"""
        N, dtc = sp.N, sp.dtc
        half = lambda t: A.View(t.data_ptr(), t.shape[3], 0)                                       # SR half (first N images)
        other = lambda t: A.View(t.data_ptr() + t[:N].numel() * t.element_size(), t.shape[3], 0)   # GT half
        sp.loss_views = (half(sp.feat), other(sp.feat))
        chain = sp.chain
        del sp.chain
        bw = []
        g = sp.g_tap = b.act(*sp.feat_dims)
        sp.keep.append(g)
        sp.dxp = b.act(sp.H, sp.W, 4, dtype=torch.float32)
        for j in range(len(chain) - 1, -1, -1):
            layer, idx, tin, tout, hh, ww, cin, cout = chain[j]
            if idx == 0:
                bw.append(b.features_to_image(sp.thin, g, sp.dxp, 4, "features.0", hh, ww, 3, cout, True, flip=True, key=("b", 0)))
                break
            gin = b.act(hh, ww, cin)
            sp.keep.append(gin)
            if layer == "conv":
                # the conv's input is a ReLU output (mask it here) or a pooled map (the pool's backward applies the ReLU')
                bw.append(b.dgrad(g, gin, ("b", idx), hh, ww, cout, cin, mask=half(tin) if chain[j - 1][0] == "conv" else A.NULL_VIEW, mask_slope=0.0))
            else:
                bw.append(ops.Call("srganfd_maxpool2_relu_bwd", (half(tin), A.view(g), A.view(gin), dtc, N, hh, ww, cin), "maxpool2_relu_bwd"))
            g = gin
        sp.bw = bw

    def forward(self, sr: Tensor, gt: Tensor) -> Tensor:
        _require_gpu(sr)
        dt, dtc = _dt(self.owner)
        dev = sr.device
        pk = self._ensure_packed(dtc, dev)
        N, Cin, H, W = sr.shape
        if Cin != 3 or H % 16 or W % 16:
            raise A.SrganfdError("ContentLoss needs 3-channel inputs with height/width multiples of 16 (four 2x2 max-pools)")
        sp = self._plan(N, H, W, dt, dtc, dev, pk, True)
        L, st = A.lib(), A.stream_ptr()
        self._load_input(sp, sr, gt, dtc, L, st)
        loss = torch.zeros(1, dtype=torch.float32, device=dev)
        ops.run_items(sp.fw, ops.Run("conv2d(vgg)", out=loss.data_ptr()))
        self.token += 1
        sp.token = self.token
        self._last = sp
        return loss.view(())

    def backward(self, sp, token, dloss: Optional[Tensor], weight: float = 1.0, upstream_ptr: Optional[int] = None) -> Tensor:
        """d(weight * loss)/d(sr) times the upstream scalar: ``dloss`` (autograd's 1-element tensor) or, for the fused trainers,
        ``upstream_ptr`` -- the address of a device float such as the loss scale -- or nothing (1)."""
        if getattr(sp, "token", None) != token:
            raise A.SrganfdError("VGG activations were overwritten by a later ContentLoss forward before backward ran")
        L, st = A.lib(), A.stream_ptr()
        N, dtc = sp.N, sp.dtc
        h, w, c = sp.feat_dims
        if dloss is not None:
            dloss = dloss.detach().contiguous().float()
            upstream_ptr = dloss.data_ptr()
        A.check(L.srganfd_l1_grad_views(sp.loss_views[0], sp.loss_views[1], A.view(sp.g_tap), dtc, N * h * w, c, upstream_ptr,
                                        weight / float(N * h * w * c), st), "l1_grad_views")
        ops.run_items(sp.bw, ops.Run("conv2d(vgg dgrad)"))
        dsr = torch.empty(N, 3, sp.H, sp.W, dtype=torch.float32, device=sp.device)
        A.check(L.srganfd_nhwc_to_nchw_scaled(A.view(sp.dxp), N, 3, sp.H, sp.W, dsr.data_ptr(), self.owner.std.data_ptr(), st), "nhwc_to_nchw_scaled")
        return dsr


class _ContentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sr, gt, eng):
        loss = eng.forward(sr, gt)
        ctx.eng, ctx.sp, ctx.token = eng, eng._last, eng.token
        return loss

    @staticmethod
    def backward(ctx, dloss):
        return ctx.eng.backward(ctx.sp, ctx.token, dloss), None, None


def content_loss_single_apply(owner: nn.Module, sr: Tensor, gt: Tensor) -> Tensor:
    eng = _engine(owner, lambda: ContentLossGradEngine(owner))
    if torch.is_grad_enabled() and sr.requires_grad:
        return _ContentFn.apply(sr, gt, eng)
    return eng.forward(sr, gt)
