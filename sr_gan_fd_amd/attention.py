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
    def _plan(self, N: int, H: int, W: int, dt, dtc: int, device, pk: dict, train: bool = True) -> _Shape:
        key = (N, H, W, dtc, str(device), pk["buf"].data_ptr(), self.fp.flat.data_ptr())
        sp = self.shapes.get(key)
        if sp is not None:
            return sp
        sp = _Shape()
        sp.N, sp.H, sp.W, sp.dt, sp.dtc, sp.device = N, H, W, dt, dtc, device
        sp.hs, sp.ws = H, W
        C, L = self.C, H * W
        V = A.view
        fptr, wptr, O = self.fp.flat.data_ptr(), pk["buf"].data_ptr(), pk["offs"]
        P = lambda name: fptr + 4 * self._poff(name)
        cv = lambda x, y, key, cin, cout, **kw: ops.Conv(ops.conv_args(dtc, V(x), V(y), wptr + O[key], N, H, W, cin, cout, ksize=1, pad=0, **kw))
        aa = lambda **kw: ops.attn_args(dtc, N, L, self.heads, self.D, qkv=sp.qkv, lse=sp.lse, **kw)

        def new(c, dtype=dt):
            return torch.empty(N, H, W, c, dtype=dtype, device=device)
        sp.xin, sp.qkv, sp.att, sp.y = new(C), new(3 * C), new(C), new(C, torch.float32)
        sp.lse = torch.empty(N, self.heads, L, dtype=torch.float32, device=device)
        sp.x_in, sp.result, sp.per_call = (V(sp.xin), C), (V(sp.y), A.F32, 0), (N, L, L)
        # the weights result is the pass's own tensor: a forward that does not want it skips the launch
        sp.fw = [cv(sp.xin, sp.qkv, ("f", "in"), C, 3 * C, bias=P(IN_B)), ops.Attention("fwd", aa(out=sp.att)), ops.PerCall(ops.Attention("weights", aa())),
                 cv(sp.att, sp.y, ("f", "out"), C, C, bias=P(OUT_B), y_f32=True)]
        # backward
        sp.dy, sp.datt, sp.dqkv, sp.dxp = new(C), new(C), new(3 * C), new(C, torch.float32)
        sp.dy_in, sp.dx_out = (V(sp.dy), C), (V(sp.dxp), A.F32)
        wplans = ops.WgradPlans(device, dtc, N)
        wg = lambda x, dy, cout, w, b: ops.Wgrad(wplans.conv(H, W, C, cout, self._poff(w), self._poff(b), ksize=1, pad=0), V(x), V(dy))
        bwd = dict(out=sp.att, d_out=sp.datt, d_qkv=sp.dqkv)
        sp.attn_ws = torch.empty(ops.attention_workspace_bytes(aa(**bwd)), dtype=torch.uint8, device=device)
        sp.bw = [wg(sp.att, sp.dy, C, OUT_W, OUT_B), cv(sp.dy, sp.datt, ("b", "out"), C, C), ops.Attention("bwd", aa(workspace=sp.attn_ws, **bwd)),
                 wg(sp.xin, sp.dqkv, 3 * C, IN_W, IN_B)]
        sp.dx_conv = cv(sp.dqkv, sp.dxp, ("b", "in"), 3 * C, C, y_f32=True)
        sp.wg_ws = wplans.workspace()
        self.shapes[key] = sp
        return sp

    def forward(self, x: Tensor, need_weights: bool) -> Tuple[Tensor, Optional[Tensor]]:
        """(attn_output (b, c, h, w), attn_output_weights (b, h*w, h*w) or None)"""
        return self._pass(x, True, per_call=need_weights)


def attention_engine(owner: nn.Module) -> AttentionEngine:
    return _engine(owner, lambda: AttentionEngine(owner))


def self_attention_apply(owner: nn.Module, x: Tensor) -> Tuple[Tensor, Optional[Tensor]]:
    """SelfAttention.forward: (attn_output (b, c, h, w), attn_output_weights (b, h*w, h*w) or None)"""
    return engine_apply(attention_engine(owner), x, bool(getattr(owner, "need_weights", True)))
