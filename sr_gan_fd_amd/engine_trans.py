"""Engine of BSRGANtrans (A-ESRGAN/model.py:643-746): the generator's engine (engine.TrunkEngine) with a stage between the trunk's
last buffer and conv2 -- one flat parameter buffer, one packed record per dtype, one forward and one backward launch list, so the
fused trainers, FlatAdamEMA and the gradient buckets reach it by the path every generator takes (engine.generator_engine).

The stage, forward (model.py:722-729):
  downsamplingTrans   3x3 stride-2 pad-1 conv + LeakyReLU(0.2) from the trunk's planar buffer into ``sp.ds`` (N, H/2, W/2, C), NHWC
  transformer_encoder ``sp.ds`` IS the (S, N, E) token tensor the reference's permute / flatten builds -- S = the batch, N = h w, token
                      (b, i, j) in row b h w + i w + j -- so the layers' lists (transformer.plan_layers) run on it as it lies: no
                      transposes, no fp32 round trip, no conversions; the last LayerNorm's output ``sp.enc_out`` is the (N, h, w, C) map
  upsamplingTrans     nearest x2 + 3x3 conv + LeakyReLU as the tail's upsampling layers run it (four parity classes in the 16-bit
                      modes, up=1 gather in fp32) into ``sp.ut``, which conv2 reads
and backward: conv2's data gradient with LeakyReLU' of ``sp.ut`` in its epilogue -> weight gradient and data gradient of
upsamplingTrans (the 4x4 stride-2 parity form / conv + nearest adjoint; its input is a LayerNorm output: no mask) -> the layers'
backward lists -> the first layer's input gradient, written in the compute type with LeakyReLU' of ``sp.ds`` in the same epilogue
(the mask is applied after the residual branch's gradient is added: the order needed) -> the (3, 2) weight-gradient plan over the
trunk's planar buffer -> the data gradient as the four parity classes of pack codes 6..9 (one class-4 launch in the 16-bit modes,
four launches in fp32) straight into channels [0, C) of the last dense block's stacked-gradient buffer.

Rounding points in the 16-bit modes, beyond the trunk's, the tail's and transformer.py's: ``sp.ds`` (the block's input: rounded once,
by the conv that writes it), ``sp.ut``; in the backward the gradient of ``sp.ut``'s pre-activation, of ``sp.enc_out`` and of
``sp.ds``'s pre-activation.  tests/bsrgantrans_oracle.py rounds at exactly these.

Dropout follows ``owner.training`` (the trainers call forward(x, True) on a module in .train(); the EMA copy and validate() run
.eval()), plans are keyed by the site probabilities, DrawMasks is the first forward item.  A forward with live dropout always takes a
plan with a backward list (the keep-masks belong to it).  An inference plan allocates no gradient buffer, no mask, and one set of
layer buffers for the whole stack.

``transformer_layer.*`` -- registered by the reference, never called -- sits in the flat buffer, is never packed or read, its range
of the flat gradient is zero (FlatParams.unwritten) and on the module path its ``.grad`` stays None (``unused_params``).
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import torch
from torch import Tensor, nn

from . import _abi as A
from . import ops
from .engine import TrunkEngine, _Shape
from .engine_core import first_layer_dgrad
from .transformer import LAYER_PARAMS, StackSite, check_layer, plan_layers

DS, UT, ENC, UNUSED = "downsamplingTrans.0", "upsamplingTrans.0", "transformer_encoder", "transformer_layer."
OPERANDS = (("in", "self_attn.in_proj_weight"), ("out", "self_attn.out_proj.weight"), ("l1", "linear1.weight"), ("l2", "linear2.weight"))


class TransGeneratorEngine(TrunkEngine):
    def __init__(self, owner: nn.Module, rdbs: Sequence[nn.Module]):
        super().__init__(owner, rdbs, rrdb=True, full=True)
        self.what = "BSRGANtrans"
        enc = owner.transformer_encoder
        if getattr(enc, "norm", None) is not None:
            raise A.SrganfdError("BSRGANtrans: a final norm on transformer_encoder has no kernel (the reference's stack has none)")
        layers = list(enc.layers)
        for layer in layers:
            check_layer(layer)
        l0 = layers[0]
        self.E, self.heads, self.F, self.eps = l0.self_attn.embed_dim, l0.self_attn.num_heads, l0.linear1.out_features, float(l0.norm1.eps)
        if self.E != self.Cc:
            raise A.SrganfdError(f"BSRGANtrans: the transformer's d_model {self.E} is not the generator's channels {self.Cc}")
        self.t_prefixes = [f"{ENC}.layers.{i}." for i in range(len(layers))]
        names = set(self.fp.names)
        for pre in self.t_prefixes:
            if any(pre + n not in names for n in LAYER_PARAMS):
                raise A.SrganfdError(f"BSRGANtrans: unexpected parameters under {pre}")
        for nm in (DS, UT):
            w = owner.get_submodule(nm).weight
            if tuple(w.shape) != (self.Cc, self.Cc, 3, 3):
                raise A.SrganfdError(f"BSRGANtrans: {nm}.weight has shape {tuple(w.shape)}, expected {(self.Cc, self.Cc, 3, 3)}")
        # the registered copy of the layer that the forward never calls
        self.unused_params = frozenset(i for i, n in enumerate(self.fp.names) if n.startswith(UNUSED))
        self.fp.unwritten = bool(self.unused_params)
        self.batch_coupled = True          # the block attends across the local batch: a sharded batch computes another function
        self._probs: tuple = ()

    # ---- dropout: the probability of every site of every layer for a forward in mode ``training`` ----
    def site_probs(self, training: bool) -> tuple:
        out = []
        for layer in self.owner.transformer_encoder.layers:
            ps = (layer.self_attn.dropout, layer.dropout1.p, layer.dropout.p, layer.dropout2.p)
            if any(not 0.0 <= p < 1.0 for p in ps):
                raise A.SrganfdError(f"{self.what}: dropout probabilities must lie in [0, 1), got {ps}")
            out.append(tuple(float(p) if training else 0.0 for p in ps))
        return tuple(out)

    def _plan_key(self) -> tuple:
        return (self._probs,)

    # ---- the input contract ----
    def trunk_size(self, shape) -> Tuple[int, int, int]:
        N, H, W = super().trunk_size(shape)
        if H % 2 or W % 2:
            raise A.SrganfdError(f"{self.what} expects even H and W (the reference's view back to (B, H / 2, W / 2, C) takes nothing else), "
                                 f"got shape {tuple(shape)}")
        if N < 1 or N > ops.SEQ_ATTN_MAX_SEQ:
            raise A.SrganfdError(f"{self.what}: batch {N} outside 1 .. {ops.SEQ_ATTN_MAX_SEQ} (the block attends over the batch: it is its sequence axis)")
        return N, H, W

    # ---- packing ----
    def _stage_pack(self, pb: ops.PackBuilder, dtc: int) -> None:
        Cc, E, F = self.Cc, self.E, self.F
        pb.fwd(("f", DS), self._poff(DS + ".weight"), Cc, Cc)
        pb.classes(("b", DS), self._poff(DS + ".weight"), Cc, Cc, 2, 6)       # 3x3 stride-2 data gradient: four parity classes of 2x2-tap convs
        for l, pre in enumerate(self.t_prefixes):
            for key, name in OPERANDS:
                co, ci = {"in": (3 * E, E), "out": (E, E), "l1": (F, E), "l2": (E, F)}[key]
                pb.fwd(("tf", l, key), self._poff(pre + name), co, ci, 1)
                pb.bwd(("tb", l, key), self._poff(pre + name), co, ci, 1)
        if self._parity(dtc):
            pb.classes(("fc", UT), self._poff(UT + ".weight"), Cc, Cc, 2, 14)
            pb.bwd(("b4", UT), self._poff(UT + ".weight"), Cc, Cc, 4, transposed=18)
        else:
            pb.fwd(("f", UT), self._poff(UT + ".weight"), Cc, Cc)
            pb.bwd(("b", UT), self._poff(UT + ".weight"), Cc, Cc)
        pb.bwd(("b", "conv1"), self._poff("conv1.weight"), Cc, self.in_ch)     # the image's gradient (the padded path; the thin kernels read the raw weight)

    # ---- plan ----
    def _stage_forward(self, sp: _Shape, b: ops.PlanBuilder, fw: list, trunk_out: A.View, train: bool) -> A.View:
        N, H, W, Cc, V = sp.N, sp.H, sp.W, self.Cc, A.view
        h, w = H // 2, W // 2
        lre = dict(act=A.ACT_LRELU, slope=0.2)
        sp.ds, sp.ut = b.act(h, w, Cc), b.act(H, W, Cc)
        fw.append(b.conv(trunk_out, sp.ds, ("f", DS), H, W, Cc, Cc, stride=2, bias=b.P(DS + ".bias"), **lre))
        T = N * h * w
        sp.g_enc = b.act(h, w, Cc) if train else None             # gradient of the stack's result
        tb = ops.PlanBuilder(self, sp, b.pk, n=1)                 # the stack's launches take the T tokens as one image
        sp.t_wplans = tb.wplans if train else None
        sp.ln_ws = b.buf(ops.add_layernorm_workspace_bytes(T, self.E), dtype=torch.uint8) if train else None
        kind = {"f": "tf", "b": "tb"}
        site = StackSite(lambda d, l, key: (kind[d], l, key), sp.ds.view(T, Cc), None if sp.g_enc is None else sp.g_enc.view(T, Cc), sp.ln_ws)
        t_fw, t_bw, out, first_dx = plan_layers(sp, tb, (self.E, self.F, self.heads, self.eps), self.t_prefixes, self._probs, N, h * w, site, train=train)
        if t_fw and t_fw[0].kind == "draw_masks":
            fw.insert(0, t_fw.pop(0))                             # DrawMasks is the first forward item
        fw.extend(t_fw)
        sp.enc_out = out.view(N, h, w, Cc)
        sp.t_len = (len(t_fw), len(t_bw))                         # how many items of each list are the stack's (tests, tools)
        if train:
            sp.g_ds = b.act(h, w, Cc)                             # gradient of downsamplingTrans's pre-activation
            # LeakyReLU' of the stack's input in the epilogue of the first layer's input gradient, after the residual branch's is added
            t_bw.append(first_dx(sp.g_ds.view(T, Cc), mask=V(sp.ds.view(T, Cc)), mask_slope=0.2))
            sp.t_bw = t_bw
        if self._parity(sp.dtc):
            fw.extend(self._up_forward(b, V(sp.enc_out), V(sp.ut), h, w, UT))
        else:
            fw.append(b.conv(sp.enc_out, sp.ut, ("f", UT), h, w, Cc, Cc, up=1, bias=b.P(UT + ".bias"), **lre))
        return V(sp.ut)

    def _conv2_dgrad_target(self, sp: _Shape, trunk_grad: A.View) -> Tuple[A.View, dict]:
        # conv2 reads upsamplingTrans's LeakyReLU output: the gradient of its pre-activation
        sp.g_ut = torch.empty_like(sp.ut)
        return A.view(sp.g_ut), dict(mask=A.view(sp.ut), mask_slope=0.2)

    def _stage_backward(self, sp: _Shape, b: ops.PlanBuilder, trunk_grad: A.View) -> list:
        N, H, W, Cc = sp.N, sp.H, sp.W, self.Cc
        h, w = H // 2, W // 2
        bw = [b.wgrad(sp.enc_out, sp.g_ut, h, w, Cc, Cc, UT + ".weight", UT + ".bias", up=1)]
        if self._parity(sp.dtc):
            it = b.dgrad(sp.g_ut, sp.g_enc, ("b4", UT), H, W, Cc, Cc, ksize=4, stride=2, pad=1)
            it.args._label_tag = " nearest-x2 dgrad"
            bw.append(it)
        else:
            sp.g_tmp = torch.empty_like(sp.ut)
            bw.append(b.dgrad(sp.g_ut, sp.g_tmp, ("b", UT), H, W, Cc, Cc))
            bw.append(b.resample(0, sp.g_tmp, sp.g_enc, h, w, Cc, what="nearest_bwd"))
        bw.extend(sp.t_bw)
        del sp.t_bw
        b.wplans.ws_bytes = max(b.wplans.ws_bytes, sp.t_wplans.ws_bytes)       # the stack's weight gradients share the list's workspace
        bw.append(b.wgrad(A.view(sp.catb(self.R), planar=sp.planar), sp.g_ds, H, W, Cc, Cc, DS + ".weight", DS + ".bias", stride=2))
        bw.extend(b.strided_dgrad(sp.g_ds, trunk_grad, ("b", DS), h, w, Cc, Cc, 2, 0))
        bw.append(ops.Ready(self._trunk_end(), self._poff("conv2.weight")))      # the stage's parameters are final, before the first dense block
        return bw

    def _trunk_end(self) -> int:
        return self._poff(DS + ".weight")

    def _finish_backward(self, sp: _Shape, b: ops.PlanBuilder) -> None:
        """the image's gradient, for a module-path backward that asks for it: conv1's data gradient, launched only then"""
        sp.dxp = b.act(sp.H, sp.W, 4, dtype=torch.float32)
        sp.dx_conv = first_layer_dgrad(b.features_to_image(sp.thin_i, sp.dx0, sp.dxp, 4, "conv1", sp.H, sp.W, self.in_ch, self.Cc, True, flip=True))
        sp.dx_out = (A.view(sp.dxp), A.F32)

    # ---- execution ----
    def forward(self, x: Tensor, train: bool) -> Tensor:
        """x: NCHW image batch.  Dropout follows the module's mode, not ``train`` (on a plan with a backward list)"""
        training = bool(self.owner.training)
        self.trunk_size(x.shape)
        self._probs = self.site_probs(training)
        live = any(p > 0 for ps in self._probs for p in ps)
        out = self._pass(x, train or live, training)[0]
        if self._last.masks:
            self._masked = self._last                    # the plan whose masks dropout_masks() reads
        return out

    def dropout_masks(self) -> Dict[str, Tensor]:
        """copies of the keep-masks of the last forward that had dropout, by ``transformer_encoder.layers.{i}.<site>`` (sites: attn
        (h w, heads, B, B), dropout1 (B, h w, C), dropout (B, h w, F), dropout2 (B, h w, C)); empty before the first such forward"""
        sp = getattr(self, "_masked", None)
        if sp is None:
            return {}
        return {k: (v.clone() if k.endswith("attn") else v.clone().view(sp.N, (sp.H // 2) * (sp.W // 2), -1)) for k, v in sp.masks.items()}
