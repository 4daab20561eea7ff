"""HIP engine of the reference's SelfAttention (BSRGAN/model.py:388-402): nn.MultiheadAttention over the h*w positions of a feature
map, every image its own sequence, no masks and no dropout.

Mapping: ``x.view(b, c, -1).permute(2, 0, 1)`` followed by the in-projection is a 1x1 convolution C -> 3C with bias over the NHWC
map -- its output IS the packed (b, h*w, 3C) q | k | v operand of the attention kernels (csrc/attention.hip), rows in in_proj_weight's
own order -- and the out-projection is a 1x1 convolution C -> C.  Both run on the implicit-GEMM kernel, their data and weight
gradients on its data-gradient form and the 1x1 weight-gradient plans, the way engine_a.py runs its gates' 1x1 convs.  No GEMM of
its own, no transposes.

This file owns the parameter checks, the packing and the plan; the passes over the plan's launch lists, the layout conversions at
their ends and the autograd glue are engine.py's (EngineBase).
Forward list:  conv 1x1 (C -> 3C), attention fwd, [attention weights: written into the forward's own tensor, skipped by a forward
               that does not want them], conv 1x1 (C -> C, fp32 out).
Backward list: wgrad(out_proj), conv 1x1 (d out -> dO), attention bwd, wgrad(in_proj); then, for a pass that wants dx, conv 1x1
               (d qkv -> dx, fp32).
Rounding points in the 16-bit modes: x, the two packed weights, qkv, P (once, for P v) and O; the output, lse, the weights result
and every accumulation are fp32.  The backward adds d out, dO and d qkv.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor, nn

from . import _abi as A
from . import ops
from .engine import EngineBase, _engine, _Shape, engine_apply

IN_W, IN_B = "multihead_attention.in_proj_weight", "multihead_attention.in_proj_bias"
OUT_W, OUT_B = "multihead_attention.out_proj.weight", "multihead_attention.out_proj.bias"


class AttentionEngine(EngineBase):
    what = "SelfAttention"

    def __init__(self, owner: nn.Module):
        super().__init__(owner, list(owner.named_parameters()))
        self.C, self.heads = owner.channels, owner.num_heads
        self.in_ch = self.out_ch = self.C
        if self.C % self.heads:
            raise A.SrganfdError(f"SelfAttention: channels {self.C} is not a multiple of num_heads {self.heads}")
        self.D = self.C // self.heads
        if self.D not in ops.ATTN_HEAD_DIMS:
            raise A.SrganfdError(f"SelfAttention: head size {self.D} (channels {self.C} / num_heads {self.heads}) has no kernel: "
                                 f"{ops.ATTN_HEAD_DIMS} have")
        if self.C % 32:
            raise A.SrganfdError(f"SelfAttention: channels {self.C} must be a multiple of 32 for the MFMA projections")
        if self.fp.names != [IN_W, IN_B, OUT_W, OUT_B]:
            raise A.SrganfdError(f"SelfAttention: unexpected parameters {self.fp.names} (kdim / vdim / bias=False are not supported)")

    def _build_pack(self, dtc: int, device) -> dict:
        pb = ops.PackBuilder(dtc)
        for key, name, co in (("in", IN_W, 3 * self.C), ("out", OUT_W, self.C)):
            pb.fwd(("f", key), self._poff(name), co, self.C, 1)
            pb.bwd(("b", key), self._poff(name), co, self.C, 1)
        return pb.finish(device)

    # ---- per-shape plan: always with its backward list ----
    always_backward = True

    def _attn_args(self, sp: _Shape, **kw):
        return ops.attn_args(sp.dtc, sp.N, sp.H * sp.W, self.heads, self.D, qkv=sp.qkv, lse=sp.lse, **kw)

    def _plan_forward(self, sp: _Shape, b: ops.PlanBuilder, train: bool) -> None:
        N, H, W, C, V = sp.N, sp.H, sp.W, self.C, A.view
        sp.hs, sp.ws = H, W
        one = dict(ksize=1, pad=0)
        sp.xin, sp.qkv, sp.att, sp.y = b.act(H, W, C), b.act(H, W, 3 * C), b.act(H, W, C), b.act(H, W, C, dtype=torch.float32)
        sp.lse = b.buf(N, self.heads, H * W, dtype=torch.float32)
        sp.x_in, sp.result, sp.per_call = (V(sp.xin), C), (V(sp.y), A.F32, 0), (N, H * W, H * W)
        # the weights result is the pass's own tensor: a forward that does not want it skips the launch
        sp.fw = [b.conv(sp.xin, sp.qkv, ("f", "in"), H, W, C, 3 * C, bias=b.P(IN_B), **one), ops.Attention("fwd", self._attn_args(sp, out=sp.att)),
                 ops.PerCall(ops.Attention("weights", self._attn_args(sp))),
                 b.conv(sp.att, sp.y, ("f", "out"), H, W, C, C, bias=b.P(OUT_B), y_f32=True, **one)]

    def _plan_backward(self, sp: _Shape, b: ops.PlanBuilder) -> None:
        H, W, C, V = sp.H, sp.W, self.C, A.view
        one = dict(ksize=1, pad=0)
        sp.dy, sp.datt, sp.dqkv, sp.dxp = b.act(H, W, C), b.act(H, W, C), b.act(H, W, 3 * C), b.act(H, W, C, dtype=torch.float32)
        sp.dy_in, sp.dx_out = (V(sp.dy), C), (V(sp.dxp), A.F32)
        bwd = dict(out=sp.att, d_out=sp.datt, d_qkv=sp.dqkv)
        sp.attn_ws = b.buf(ops.attention_workspace_bytes(self._attn_args(sp, **bwd)), dtype=torch.uint8)
        sp.bw = [b.wgrad(sp.att, sp.dy, H, W, C, C, OUT_W, OUT_B, **one), b.dgrad(sp.dy, sp.datt, ("b", "out"), H, W, C, C, **one),
                 ops.Attention("bwd", self._attn_args(sp, workspace=sp.attn_ws, **bwd)), b.wgrad(sp.xin, sp.dqkv, H, W, C, 3 * C, IN_W, IN_B, **one)]
        sp.dx_conv = b.dgrad(sp.dqkv, sp.dxp, ("b", "in"), H, W, 3 * C, C, y_f32=True, **one)
        sp.wg_ws = b.wplans.workspace()

    def forward(self, x: Tensor, need_weights: bool) -> Tuple[Tensor, Optional[Tensor]]:
        """(attn_output (b, c, h, w), attn_output_weights (b, h*w, h*w) or None)"""
        return self._pass(x, True, per_call=need_weights)


def attention_engine(owner: nn.Module) -> AttentionEngine:
    return _engine(owner, lambda: AttentionEngine(owner))


def self_attention_apply(owner: nn.Module, x: Tensor) -> Tuple[Tensor, Optional[Tensor]]:
    """SelfAttention.forward: (attn_output (b, c, h, w), attn_output_weights (b, h*w, h*w) or None)"""
    return engine_apply(attention_engine(owner), x, bool(getattr(owner, "need_weights", True)))
