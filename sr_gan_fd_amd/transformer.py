"""HIP engine of the reference's transformer block (A-ESRGAN/model.py:673-674, called at :725-726): a stack of post-norm
nn.TransformerEncoderLayer (norm_first=False, ReLU, biases everywhere, LayerNorm eps 1e-5, no final norm, no masks) over a
``(S, N, E)`` tensor with batch_first=False -- S is the sequence axis.  The reference feeds it ``(B, h w, C)``, so every pixel
position is a "batch" entry that attends over the B images of the training batch; the engine reproduces that and repairs nothing.

Mapping: ``(S, N, E)`` contiguous is token-major, token (s, n) in row s N + n -- the NHWC feature map (B, h, w, C) of a later
BSRGANtrans with S = B and N = h w.  What works per token does not care about the order of the tokens: the in-projection E -> 3E, the
out-projection, linear1 (+ ReLU in the epilogue) and linear2 are 1x1 launches of the implicit-GEMM kernel over a (1, S, N) map, their
data gradients its data-gradient form (linear1's with the ReLU' mask epilogue over the stored hidden activation, and with the
residual branch's gradient added in the epilogue), their weight gradients the 1x1 weight-gradient plans -- as attention.py does.  The
attention itself runs on csrc/attention_seq.hip, which reads the (S, N, 3E) in-projection output with a token stride of N rows: no
transposes.  Residual add + its dropout + LayerNorm is one launch (csrc/layernorm.hip), forward and backward.

Dropout (``training`` with p > 0): four sites per layer -- the attention probabilities (nseq, heads, S, S), dropout1 on the
out-projection output, the feed-forward dropout on the hidden activation, dropout2 on linear2's output.  The keep-masks are uint8
tensors owned by the plan and refilled by torch (``bernoulli_``: they follow torch.manual_seed and are safe under graph capture) by the
first item of the forward list; the kernels multiply by keep / (1 - p) in the forward pass and read the same masks in the backward
pass.  Eval mode, or p = 0 at a site: no mask, no launch for it.

This file owns the parameter checks, the packing and the plan; the passes over the plan's launch lists, the conversions at their
ends and the autograd glue are engine.py's (EngineBase): the tokens enter and leave as a (S N, E, 1, 1) "image", for which the
boundary kernels are plain dtype conversions.
Forward list, per layer:  [draw masks]  conv 1x1 (E -> 3E), seq attention fwd, conv 1x1 (E -> E), add + LayerNorm (norm1),
               conv 1x1 (E -> F, ReLU), [dropout], conv 1x1 (F -> E), add + LayerNorm (norm2).
Backward list, per layer, last layer first: add + LayerNorm bwd (norm2: dz -> the residual branch, dr, dgamma, dbeta),
               wgrad(linear2), conv 1x1 (dr -> d hidden, ReLU' mask), [dropout], wgrad(linear1), conv 1x1 (d hidden -> d y1, + dz),
               add + LayerNorm bwd (norm1), wgrad(out_proj), conv 1x1 (-> dO), seq attention bwd, wgrad(in_proj),
               conv 1x1 (d qkv -> the layer input's gradient, + dz; the first layer's only for a pass that wants d src, fp32).
Rounding points in the 16-bit modes: the input; the packed weights (biases, gamma and beta stay fp32); qkv; P (once, before the
keep-mask) and O; the out-projection's and linear2's outputs; both z = x + dropout(r), whose STORED value LayerNorm normalises; both
LayerNorm outputs (the last one is the result, converted back to fp32); the hidden activation.  lse, mean, rstd and every
accumulation are fp32.  The backward adds every stored gradient: d out, both dz and dr, d hidden, d y1, dO, d qkv and the gradient
between two layers.  tests/transformer_oracle.py rounds at exactly these points.
"""
from __future__ import annotations

from typing import Callable, Dict, NamedTuple, Optional, Sequence, Tuple

import torch
from torch import Tensor, nn

from . import _abi as A
from . import ops
from .engine import EngineBase, _engine, _Shape, engine_apply

LAYER_PARAMS = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
                "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")
SITES = ("attn", "dropout1", "dropout", "dropout2")        # the four dropout sites of a layer, in forward order


def check_layer(layer: nn.TransformerEncoderLayer) -> None:
    """what of nn.TransformerEncoderLayer's options has a kernel: raises SrganfdError for the rest, before anything is planned"""
    what = "TransformerEncoderLayer"
    if getattr(layer, "norm_first", False):
        raise A.SrganfdError(f"{what}: norm_first=True has no kernel (the reference's block is post-norm)")
    act = layer.activation
    if not (act is torch.nn.functional.relu or isinstance(act, nn.ReLU)):
        raise A.SrganfdError(f"{what}: activation {getattr(act, '__name__', act)!r} has no kernel (ReLU has)")
    if layer.self_attn.batch_first:
        raise A.SrganfdError(f"{what}: batch_first=True has no kernel (the reference's block takes (S, N, E))")
    if [n for n, _ in layer.named_parameters()] != list(LAYER_PARAMS):
        raise A.SrganfdError(f"{what}: unexpected parameters {[n for n, _ in layer.named_parameters()]} (bias=False, kdim and vdim are not supported)")
    E, heads, F = layer.self_attn.embed_dim, layer.self_attn.num_heads, layer.linear1.out_features
    if E % 32:
        raise A.SrganfdError(f"{what}: d_model {E} must be a multiple of 32 for the MFMA projections")
    if E % heads or E // heads not in ops.ATTN_HEAD_DIMS:
        raise A.SrganfdError(f"{what}: head size d_model {E} / nhead {heads} has no kernel: {ops.ATTN_HEAD_DIMS} have")
    if F % 32:
        raise A.SrganfdError(f"{what}: dim_feedforward {F} must be a multiple of 32 for the MFMA projections")


def check_no_masks(what: str, **given) -> None:
    for name, v in given.items():
        if v is not None and v is not False:
            raise A.SrganfdError(f"{what}: {name} is not supported (the reference's block passes no mask)")


class DrawMasks:
    """first item of a training plan's forward list: refills the plan's keep-masks, on the stream the kernels run on.  torch draws
    them -- they follow torch.manual_seed, and under graph capture every replay draws new ones."""
    kind = "draw_masks"

    def __init__(self, masks: Sequence[Tuple[Tensor, float]]):
        self.masks = list(masks)

    def launch(self, run: ops.Run) -> None:
        if not A.DRY_RUN:
            for t, p in self.masks:
                t.bernoulli_(1.0 - p)


class StackSite(NamedTuple):
    """where a stack of layers sits in its engine (plan_layers): ``key(d, l, k)``: the pack key of layer l's operand ``k`` ("in",
    "out", "l1", "l2"), forward (d "f") or data-gradient (d "b") orientation; ``x_in`` (T, E): the first layer's input; ``dy`` (T, E):
    the gradient of the last layer's output; ``ln_ws``: the engine's add + LayerNorm workspace (the last two None for an inference
    plan)"""
    key: Callable
    x_in: Tensor
    dy: Optional[Tensor]
    ln_ws: Optional[Tensor]


def plan_layers(sp: _Shape, pb: ops.PlanBuilder, dims: tuple, prefixes: Sequence[str], probs: tuple, S: int, Nq: int, site: StackSite, train: bool = True):
    """The launch lists of a stack of layers over T = S Nq tokens, for the stand-alone engine below and for the generator that holds
    the stack between its trunk and its tail (engine_trans.py).  ``pb``: a plan builder with a batch of 1 -- the tokens are one
    (S, Nq) image to the 1x1 convs -- whose weight-gradient plans are the stack's; ``dims``: (E, F, heads, eps); ``prefixes``: the
    layers' parameter prefixes; ``probs``: site_probs'; ``site``: where the stack sits (StackSite).
    Sets sp.layers (the layers' buffers) and sp.masks ({"<prefix><site>": keep-mask}); returns (forward items -- DrawMasks first when
    a site has p > 0 --, backward items without the first layer's input gradient, the buffer of the stack's output, ``first_dx``:
    ``first_dx(y, **epilogue)`` makes the item that writes the first layer's input gradient into ``y``).
    ``train`` False (an inference plan; no site may have p > 0): no backward list, and one set of buffers serves every layer -- the
    kernels' z, mean, rstd and lse outputs, which only a backward pass reads, land in that one set too."""
    E, F, heads, eps = dims
    key, x_in, dy, ln_ws = site
    D, T = E // heads, S * Nq
    V, dtc, device = A.view, pb.dtc, pb.device
    conv1 = lambda x, y, k, cin, cout, **kw: pb.conv(x, y, key(*k), S, Nq, cin, cout, ksize=1, pad=0, **kw)
    tok = lambda c: pb.buf(T, c)                     # a (T, c) buffer of the stack
    stat = lambda: pb.buf(T, dtype=torch.float32)
    u8 = lambda *shape: torch.ones(*shape, dtype=torch.uint8, device=device)
    sp.layers, sp.masks = [], {}
    fw, bw, draws = [], [], []
    L = len(prefixes)
    dxs = [tok(E) if (l > 0 and train) else None for l in range(L)]      # the gradient between two layers: layer l's input is layer l - 1's output
    x_l = x_in                                       # a layer's input
    per_layer_bw, first_dx = [], None
    for l, pre in enumerate(prefixes):
        off = lambda name: pb.poff(pre + name)
        if train or l == 0:
            b = _Shape()                             # the layer's buffers
            b.qkv, b.att, b.a, b.z1, b.y1, b.hid, b.f, b.z2, b.y2 = tok(3 * E), tok(E), tok(E), tok(E), tok(E), tok(F), tok(E), tok(E), tok(E)
            b.lse = torch.empty(Nq, heads, S, dtype=torch.float32, device=device)
            b.mean1, b.rstd1, b.mean2, b.rstd2 = stat(), stat(), stat(), stat()
        else:
            prev, b = b, _Shape()                    # inference: the one set again, the output in the buffer the layer does not read
            b.__dict__.update(prev.__dict__)
            b.y2 = sp.layers[l - 2].y2 if l >= 2 else tok(E)
        sp.layers.append(b)
        shapes = {"attn": (Nq, heads, S, S), "dropout1": (T, E), "dropout": (T, F), "dropout2": (T, E)}
        keep, scale = {}, {}
        for site, p in zip(SITES, probs[l]):
            keep[site], scale[site] = (u8(*shapes[site]), 1.0 / (1.0 - p)) if p > 0 else (None, 1.0)
            if p > 0:
                if not train:
                    raise A.SrganfdError("dropout needs a plan with a backward list (the keep-masks belong to it)")
                sp.masks[pre + site] = keep[site]
                draws.append((keep[site], p))
        aa = lambda **kw: ops.seq_attn_args(dtc, S, Nq, heads, D, qkv=b.qkv, out=b.att, lse=b.lse, keep=keep["attn"], keep_scale=scale["attn"], **kw)
        ln = lambda **kw: ops.AddLayerNorm(dtc, T, E, eps=eps, **kw)
        fw += [conv1(x_l, b.qkv, ("f", l, "in"), E, 3 * E, bias=pb.P(pre + "self_attn.in_proj_bias")), ops.SeqAttention("fwd", aa()),
               conv1(b.att, b.a, ("f", l, "out"), E, E, bias=pb.P(pre + "self_attn.out_proj.bias")),
               ln(x=x_l, r=b.a, keep=keep["dropout1"], keep_scale=scale["dropout1"], gamma=pb.P(pre + "norm1.weight"), beta=pb.P(pre + "norm1.bias"), z=b.z1, y=b.y1,
                  mean=b.mean1, rstd=b.rstd1),
               conv1(b.y1, b.hid, ("f", l, "l1"), E, F, bias=pb.P(pre + "linear1.bias"), act=A.ACT_RELU)]
        if keep["dropout"] is not None:
            fw.append(ops.DropoutApply(dtc, b.hid, keep["dropout"], scale["dropout"], b.hid, T * F))
        fw += [conv1(b.hid, b.f, ("f", l, "l2"), F, E, bias=pb.P(pre + "linear2.bias")),
               ln(x=b.y1, r=b.f, keep=keep["dropout2"], keep_scale=scale["dropout2"], gamma=pb.P(pre + "norm2.weight"), beta=pb.P(pre + "norm2.bias"), z=b.z2, y=b.y2,
                  mean=b.mean2, rstd=b.rstd2)]
        x_in_l, x_l = x_l, b.y2
        if not train:
            continue
        # backward of the layer, from dy_l (the gradient of y2) to the gradient of its input
        dy_l = dxs[l + 1] if l + 1 < L else dy       # the gradient of the layer's output
        b.dz2, b.df, b.dhid, b.dy1, b.dz1, b.da, b.datt, b.dqkv = tok(E), tok(E), tok(F), tok(E), tok(E), tok(E), tok(E), tok(3 * E)
        b.dx = dxs[l]
        wg1 = lambda x, dy, cin, cout, w, bias: pb.wgrad(x, dy, S, Nq, cin, cout, pre + w, pre + bias, ksize=1, pad=0)
        lb = [ln(dy=dy_l, z=b.z2, mean=b.mean2, rstd=b.rstd2, gamma=pb.P(pre + "norm2.weight"), keep=keep["dropout2"], keep_scale=scale["dropout2"], dx=b.dz2,
                 dr=b.df, dg_off=off("norm2.weight"), db_off=off("norm2.bias"), ws=ln_ws),
              wg1(b.hid, b.df, F, E, "linear2.weight", "linear2.bias"),
              conv1(b.df, b.dhid, ("b", l, "l2"), E, F, mask=V(b.hid), mask_slope=0.0)]
        if keep["dropout"] is not None:
            lb.append(ops.DropoutApply(dtc, b.dhid, keep["dropout"], scale["dropout"], b.dhid, T * F))
        lb += [wg1(b.y1, b.dhid, E, F, "linear1.weight", "linear1.bias"),
               conv1(b.dhid, b.dy1, ("b", l, "l1"), F, E, r1=V(b.dz2), r1_scale=1.0),
               ln(dy=b.dy1, z=b.z1, mean=b.mean1, rstd=b.rstd1, gamma=pb.P(pre + "norm1.weight"), keep=keep["dropout1"], keep_scale=scale["dropout1"], dx=b.dz1,
                  dr=b.da, dg_off=off("norm1.weight"), db_off=off("norm1.bias"), ws=ln_ws),
               wg1(b.att, b.da, E, E, "self_attn.out_proj.weight", "self_attn.out_proj.bias"),
               conv1(b.da, b.datt, ("b", l, "out"), E, E),
               ops.SeqAttention("bwd", aa(d_out=b.datt, d_qkv=b.dqkv)),
               wg1(x_in_l, b.dqkv, E, 3 * E, "self_attn.in_proj_weight", "self_attn.in_proj_bias")]
        if l > 0:
            lb.append(conv1(b.dqkv, b.dx, ("b", l, "in"), 3 * E, E, r1=V(b.dz1), r1_scale=1.0))
        else:
            first_dx = lambda y, b=b, **kw: conv1(b.dqkv, y, ("b", 0, "in"), 3 * E, E, r1=V(b.dz1), r1_scale=1.0, **kw)
        per_layer_bw.append(lb)
    for lb in reversed(per_layer_bw):
        bw += lb
    if draws:
        fw.insert(0, DrawMasks(draws))
    return fw, bw, x_l, first_dx


class TransformerEngine(EngineBase):
    what = "TransformerEncoder"

    def __init__(self, owner: nn.Module, layers: Sequence[nn.Module], prefixes: Sequence[str]):
        super().__init__(owner, list(owner.named_parameters()))
        for layer in layers:
            check_layer(layer)
        l0 = layers[0]
        self.prefixes = list(prefixes)
        self.E, self.heads, self.F, self.eps = l0.self_attn.embed_dim, l0.self_attn.num_heads, l0.linear1.out_features, float(l0.norm1.eps)
        self.D = self.E // self.heads
        self.in_ch = self.out_ch = self.E
        if self.fp.names != [pre + n for pre in self.prefixes for n in LAYER_PARAMS]:
            raise A.SrganfdError(f"{self.what}: unexpected parameters {self.fp.names}")
        self._call: Tuple[int, int, tuple] = (0, 0, ())

    def site_probs(self, training: bool) -> tuple:
        """the dropout probability of every site of every layer for a forward in mode ``training`` (all 0 in eval mode), read from the
        layers at call time: ((attn, dropout1, dropout, dropout2), ...)"""
        out = []
        for pre in self.prefixes:
            layer = self.owner.get_submodule(pre[:-1]) if pre else self.owner
            ps = (layer.self_attn.dropout, layer.dropout1.p, layer.dropout.p, layer.dropout2.p)
            if any(not 0.0 <= p < 1.0 for p in ps):
                raise A.SrganfdError(f"{self.what}: dropout probabilities must lie in [0, 1), got {ps}")
            out.append(tuple(float(p) if training else 0.0 for p in ps))
        return tuple(out)

    def _build_pack(self, dtc: int, device) -> dict:
        pb = ops.PackBuilder(dtc)
        E, F = self.E, self.F
        for l, pre in enumerate(self.prefixes):
            for key, name, co, ci in (("in", "self_attn.in_proj_weight", 3 * E, E), ("out", "self_attn.out_proj.weight", E, E),
                                      ("l1", "linear1.weight", F, E), ("l2", "linear2.weight", E, F)):
                pb.fwd(("f", l, key), self._poff(pre + name), co, ci, 1)
                pb.bwd(("b", l, key), self._poff(pre + name), co, ci, 1)
        return pb.finish(device)

    # ---- per-shape plan: always with its backward list; T tokens enter as a (T, E, 1, 1) image (see forward) ----
    always_backward = True
    conv_batch = 1

    def _plan_key(self) -> tuple:
        return self._call

    def _plan_forward(self, sp: _Shape, b: ops.PlanBuilder, train: bool) -> None:
        """both halves: plan_layers makes a layer's backward items beside its forward items"""
        S, Nq, probs = self._call
        T, E, V = sp.N, self.E, A.view
        assert T == S * Nq and sp.H == sp.W == 1
        sp.hs = sp.ws = 1
        sp.S, sp.Nq = S, Nq
        sp.ln_ws = b.buf(ops.add_layernorm_workspace_bytes(T, E), dtype=torch.uint8)
        sp.xin = b.buf(T, E)
        sp.dy = b.buf(T, E)                                   # gradient of the stack's result
        sp.dxp = b.buf(T, E, dtype=torch.float32)             # gradient of its input
        site = StackSite(lambda d, l, k: (d, l, k), sp.xin, sp.dy, sp.ln_ws)
        sp.fw, sp.bw, out, first_dx = plan_layers(sp, b, (self.E, self.F, self.heads, self.eps), self.prefixes, probs, S, Nq, site)
        sp.dx_conv = first_dx(sp.dxp, y_f32=True)        # the first layer's: only for a pass that wants d src, fp32
        sp.x_in, sp.result = (V(sp.xin), E), (V(out), sp.dtc, 0)
        sp.dy_in, sp.dx_out = (V(sp.dy), E), (V(sp.dxp), A.F32)
        sp.wg_ws = b.wplans.workspace()

    def _plan_backward(self, sp: _Shape, b: ops.PlanBuilder) -> None:
        """(made by _plan_forward)"""

    def forward(self, x: Tensor, training: bool) -> Tensor:
        """x (S, N, E); always on a plan with a backward list, in the module's mode ``training``"""
        if x.dim() != 3 or x.shape[-1] != self.E:
            raise A.SrganfdError(f"{self.what} expects (S, N, {self.E}) inputs, got shape {tuple(x.shape)}")
        S, Nq = x.shape[0], x.shape[1]
        if S < 1 or Nq < 1 or S > ops.SEQ_ATTN_MAX_SEQ:
            raise A.SrganfdError(f"{self.what}: sequence length {S} outside 1 .. {ops.SEQ_ATTN_MAX_SEQ} (the reference's sequence axis is its batch)")
        self._call = (S, Nq, self.site_probs(training))
        out = self._pass(x.contiguous().reshape(S * Nq, self.E, 1, 1), True, training)[0]
        if self._last.masks:
            self._masked = self._last                    # the plan whose masks dropout_masks() reads
        return out.view(S, Nq, self.E)

    def backward(self, sp: _Shape, token: int, dout: Tensor, need_wgrad: bool, need_dx: bool, on_ready=None):
        g, dx = super().backward(sp, token, dout, need_wgrad, need_dx, on_ready)
        return g, (None if dx is None else dx.view(sp.S, sp.Nq, self.E))

    def dropout_masks(self) -> Dict[str, Tensor]:
        """copies of the keep-masks of the last forward that had dropout, by ``<layer prefix><site>`` (sites: attn (N, heads, S, S),
        dropout1 (S, N, E), dropout (S, N, F), dropout2 (S, N, E)); empty before the first such forward"""
        sp = getattr(self, "_masked", None)
        if sp is None:
            return {}
        return {k: (v.clone() if k.endswith("attn") else v.clone().view(sp.S, sp.Nq, -1)) for k, v in sp.masks.items()}


def transformer_engine(owner: nn.Module) -> TransformerEngine:
    def make():
        if isinstance(owner, nn.TransformerEncoder):
            if owner.norm is not None:
                raise A.SrganfdError("TransformerEncoder: a final norm has no kernel (the reference's stack has none)")
            return TransformerEngine(owner, list(owner.layers), [f"layers.{i}." for i in range(len(owner.layers))])
        return TransformerEngine(owner, [owner], [""])            # the lone layer is a one-layer stack
    return _engine(owner, make)


def transformer_apply(owner: nn.Module, src: Tensor) -> Tensor:
    """forward of model.TransformerEncoderLayer / model.TransformerEncoder: (S, N, E) fp32 -> the same"""
    return engine_apply(transformer_engine(owner), src, bool(owner.training))
