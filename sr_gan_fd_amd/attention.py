"""HIP engine of the reference's SelfAttention (BSRGAN/model.py:388-402): nn.MultiheadAttention over the h*w positions of a feature
map, every image its own sequence, no masks and no dropout.

Mapping: ``x.view(b, c, -1).permute(2, 0, 1)`` followed by the in-projection is a 1x1 convolution C -> 3C with bias over the NHWC
map -- its output IS the packed (b, h*w, 3C) q | k | v operand of the attention kernels (csrc/attention.hip), rows in in_proj_weight's
own order -- and the out-projection is a 1x1 convolution C -> C.  Both run on the implicit-GEMM kernel, their data and weight
gradients on its data-gradient form and the 1x1 weight-gradient plans, the way engine_a.py runs its gates' 1x1 convs.  No GEMM of
its own, no transposes.

Forward:  nchw_to_nhwc, conv 1x1 (C -> 3C), attention_fwd, [attention_weights], conv 1x1 (C -> C, fp32 out), nhwc_to_nchw.
Backward: nchw_to_nhwc(d out), wgrad(out_proj), conv 1x1 (d out -> dO), attention_bwd, wgrad(in_proj), conv 1x1 (d qkv -> dx, fp32),
          nhwc_to_nchw.
Rounding points in the 16-bit modes: x, the two packed weights, qkv, P (once, for P v) and O; the output, lse, the weights result
and every accumulation are fp32.  The backward adds d out, dO and d qkv.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor, nn

from . import _abi as A
from . import ops
from . import profiling
from .engine import EngineBase, _dt, _engine, _require_gpu, _Shape, check_channels

IN_W, IN_B = "multihead_attention.in_proj_weight", "multihead_attention.in_proj_bias"
OUT_W, OUT_B = "multihead_attention.out_proj.weight", "multihead_attention.out_proj.bias"


class AttentionEngine(EngineBase):
    def __init__(self, owner: nn.Module):
        super().__init__(owner, list(owner.named_parameters()))
        self.C, self.heads = owner.channels, owner.num_heads
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

    # ---- per-shape plan ----
    def _plan(self, N: int, H: int, W: int, dt, dtc: int, device, pk: dict) -> _Shape:
        key = (N, H, W, dtc, str(device), pk["buf"].data_ptr(), self.fp.flat.data_ptr())
        sp = self.shapes.get(key)
        if sp is not None:
            return sp
        sp = _Shape()
        sp.N, sp.H, sp.W, sp.dt, sp.dtc, sp.device = N, H, W, dt, dtc, device
        C, L = self.C, H * W
        V = A.view
        fptr, wptr, O = self.fp.flat.data_ptr(), pk["buf"].data_ptr(), pk["offs"]
        P = lambda name: fptr + 4 * self._poff(name)

        def new(c, dtype=dt):
            return torch.empty(N, H, W, c, dtype=dtype, device=device)
        sp.xin, sp.qkv, sp.att, sp.y = new(C), new(3 * C), new(C), new(C, torch.float32)
        sp.lse = torch.empty(N, self.heads, L, dtype=torch.float32, device=device)
        sp.in_conv = ops.conv_args(dtc, V(sp.xin), V(sp.qkv), wptr + O[("f", "in")], N, H, W, C, 3 * C, ksize=1, pad=0, bias=P(IN_B))
        sp.attn = ops.attn_args(dtc, N, L, self.heads, self.D, qkv=sp.qkv, out=sp.att, lse=sp.lse)
        sp.out_conv = ops.conv_args(dtc, V(sp.att), V(sp.y), wptr + O[("f", "out")], N, H, W, C, C, ksize=1, pad=0, bias=P(OUT_B), y_f32=True)
        # backward
        sp.dy, sp.datt, sp.dqkv, sp.dxp = new(C), new(C), new(3 * C), new(C, torch.float32)
        wplans = ops.WgradPlans(device, dtc, N)
        sp.out_wgrad = wplans.conv(H, W, C, C, self._poff(OUT_W), self._poff(OUT_B), ksize=1, pad=0)
        sp.in_wgrad = wplans.conv(H, W, C, 3 * C, self._poff(IN_W), self._poff(IN_B), ksize=1, pad=0)
        sp.wg_ws = wplans.workspace()
        sp.out_dgrad = ops.conv_args(dtc, V(sp.dy), V(sp.datt), wptr + O[("b", "out")], N, H, W, C, C, ksize=1, pad=0)
        sp.in_dgrad = ops.conv_args(dtc, V(sp.dqkv), V(sp.dxp), wptr + O[("b", "in")], N, H, W, 3 * C, C, ksize=1, pad=0, y_f32=True)
        bw = ops.attn_args(dtc, N, L, self.heads, self.D, qkv=sp.qkv, out=sp.att, lse=sp.lse, d_out=sp.datt, d_qkv=sp.dqkv)
        sp.attn_ws = torch.empty(ops.attention_workspace_bytes(bw), dtype=torch.uint8, device=device)
        sp.attn_bwd = ops.attn_args(dtc, N, L, self.heads, self.D, qkv=sp.qkv, out=sp.att, lse=sp.lse, d_out=sp.datt, d_qkv=sp.dqkv,
                                    workspace=sp.attn_ws)
        self.shapes[key] = sp
        return sp

    # ---- execution ----
    def forward(self, x: Tensor, need_weights: bool) -> Tuple[Tensor, Optional[Tensor]]:
        check_channels("SelfAttention", x, self.C)
        _require_gpu(x)
        dt, dtc = _dt(self.owner)
        dev = x.device
        pk = self._ensure_packed(dtc, dev)
        N, C, H, W = x.shape
        sp = self._plan(N, H, W, dt, dtc, dev, pk)
        L, st, rec = A.lib(), A.stream_ptr(), profiling.REC
        x = x.contiguous().float()
        A.check(L.srganfd_nchw_to_nhwc(x.data_ptr(), N, C, H, W, A.view(sp.xin), dtc, C, None, None, st), "nchw_to_nhwc")
        ops.conv2d(sp.in_conv, rec, "conv2d(in_proj)", L, st)
        ops.attention_fwd(sp.attn, rec, L, st)
        weights = None
        if need_weights:
            weights = torch.empty(N, H * W, H * W, dtype=torch.float32, device=dev)
            ops.attention_weights(ops.attn_args(dtc, N, H * W, self.heads, self.D, qkv=sp.qkv, lse=sp.lse, weights=weights), rec, L, st)
        ops.conv2d(sp.out_conv, rec, "conv2d(out_proj)", L, st)
        out = torch.empty(N, C, H, W, dtype=torch.float32, device=dev)
        A.check(L.srganfd_nhwc_to_nchw(A.view(sp.y), A.F32, N, C, H, W, out.data_ptr(), 0, st), "nhwc_to_nchw")
        self.token += 1
        sp.token = self.token
        self._last = sp
        return out, weights

    def backward(self, sp: _Shape, token: int, dout: Tensor, need_wgrad: bool, need_dx: bool) -> Tuple[Optional[Tensor], Optional[Tensor]]:
        if getattr(sp, "token", None) != token:
            raise A.SrganfdError("SelfAttention activations were overwritten by a later forward of the same module before backward ran")
        L, st, rec = A.lib(), A.stream_ptr(), profiling.REC
        N, H, W, C, dtc = sp.N, sp.H, sp.W, self.C, sp.dtc
        V = A.view
        dout = dout.contiguous().float()
        A.check(L.srganfd_nchw_to_nhwc(dout.data_ptr(), N, C, H, W, V(sp.dy), dtc, C, None, None, st), "nchw_to_nhwc")
        flat_grad = self.fp.new_grad(sp.device) if need_wgrad else None
        if need_wgrad:
            ops.conv2d_wgrad(sp.out_wgrad, V(sp.att), V(sp.dy), flat_grad.data_ptr(), sp.wg_ws, rec, L, st)
        ops.conv2d(sp.out_dgrad, rec, "conv2d(dgrad out_proj)", L, st)
        ops.attention_bwd(sp.attn_bwd, rec, L, st)
        if need_wgrad:
            ops.conv2d_wgrad(sp.in_wgrad, V(sp.xin), V(sp.dqkv), flat_grad.data_ptr(), sp.wg_ws, rec, L, st)
        dx = None
        if need_dx:
            ops.conv2d(sp.in_dgrad, rec, "conv2d(dgrad in_proj)", L, st)
            dx = torch.empty(N, C, H, W, dtype=torch.float32, device=sp.device)
            A.check(L.srganfd_nhwc_to_nchw(V(sp.dxp), A.F32, N, C, H, W, dx.data_ptr(), 0, st), "nhwc_to_nchw")
        return flat_grad, dx


class _AttentionFn(torch.autograd.Function):
    """differentiable in the attention output only; the weights result is handed over beside it, detached (module docstring)"""

    @staticmethod
    def forward(ctx, x, eng, need_weights, box, *params):
        out, box["weights"] = eng.forward(x, need_weights)
        ctx.eng, ctx.sp, ctx.token = eng, eng._last, eng.token
        ctx.need_dx = ctx.needs_input_grad[0]
        ctx.need_w = any(ctx.needs_input_grad[4:])
        return out

    @staticmethod
    def backward(ctx, dout):
        g, dx = ctx.eng.backward(ctx.sp, ctx.token, dout, ctx.need_w, ctx.need_dx)
        grads = tuple(ctx.eng.fp.grad_views(g)) if g is not None else tuple(None for _ in ctx.eng.fp.params)
        return (dx, None, None, None) + grads


def attention_engine(owner: nn.Module) -> AttentionEngine:
    return _engine(owner, lambda: AttentionEngine(owner))


def self_attention_apply(owner: nn.Module, x: Tensor) -> Tuple[Tensor, Optional[Tensor]]:
    """SelfAttention.forward: (attn_output (b, c, h, w), attn_output_weights (b, h*w, h*w) or None)"""
    eng = attention_engine(owner)
    need_weights = bool(getattr(owner, "need_weights", True))
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in eng.fp.params)):
        box = {}
        out = _AttentionFn.apply(x, eng, need_weights, box, *eng.fp.params)
        return out, box["weights"]
    return eng.forward(x, need_weights)
