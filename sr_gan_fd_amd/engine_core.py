"""What the three discriminator engines (engine_d.py, engine_a.py, engine_e.py) share: spectral-norm state and packing, the
forward and backward passes over the launch lists, and the autograd glue.

A subclass describes its network: the layer tables, ``_build_pack``, ``_plan`` / ``_plan_backward`` (the launch lists) and, beside
itself, the launch items only it has (BatchNorm).  A plan ``sp`` carries (items: ops.py's, each with ``launch(run)``)
  sp.xin                 NHWC input buffer (4-channel pitch for the thin kernels, else padded to 32)
  sp.fw                  forward items: ops.Conv | ops.ThinLaunch | ops.Call | the engine's own; the last one, an ops.PerCall, writes
                         the fp32 logits (allocated per forward: ``run.out``)
  sp.dl                  NHWC buffer of the logits' gradient
  sp.bw                  backward items: the forward kinds and ops.Wgrad (``sn``: the layer's spectral-norm slot, or None); the last
                         one is the SnGradBatch ``_backward_workspaces`` appends
  sp.dx_conv, sp.dxp     the item (``first_layer_dgrad``) of the first layer's data gradient and its fp32 NHWC4 output
  sp.wg_ws, sp.gtmp      workspaces (``_backward_workspaces``)
"""
from __future__ import annotations

import ctypes as C
import weakref
from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor, nn

from . import _abi as A
from . import ops
from .engine import EngineBase, _dt, _require_gpu, _Shape, check_channels


class SnGradBatch:
    """Last item of a backward list: dL/d(W/sigma) of every spectral-normalised layer sits in its own range of the scratch gradient,
    and one batched pass turns them into dL/dW_orig in the flat gradient.  ``layers``: the spectral-norm slots of the list's Wgrad
    items; ``inv_sigma``: the packed record's scalars; nothing to do for a pass with frozen parameters (no Wgrad ran)."""
    kind = "sn_grad"

    def __init__(self, eng: "DiscriminatorEngineCore", layers: Sequence[int], inv_sigma: Optional[Tensor], ws: Tensor):
        self.eng, self.layers, self.inv_sigma, self.ws = weakref.proxy(eng), list(layers), inv_sigma, ws     # (a plan must not hold its engine)

    def launch(self, run: ops.Run) -> None:
        if not (run.need_wgrad and self.layers):
            return
        eng, jobs = self.eng, []
        flat, isig = eng.fp.flat.data_ptr(), self.inv_sigma.data_ptr()
        for l in self.layers:
            name, rows, cols = eng.sn[l]
            off = 4 * eng._poff(name)
            u, v = eng._sn_uv(l)
            jobs.append((run.scratch + off, flat + off, u.data_ptr(), v.data_ptr(), isig + 4 * (2 * l + 1), run.grad + off, rows, cols))
        ops.spectral_norm_grad_batch(jobs, self.ws)


def first_layer_dgrad(item):
    """sp.dx_conv from the item of the first layer's data gradient (launched only by a pass that wants the input's gradient): the
    conv is never bracketed (its thin twin is) and reported under a name of its own"""
    if isinstance(item, ops.Conv):
        return ops.Call("srganfd_conv2d", (C.byref(item.args),), "conv2d(dgrad of the first layer)")      # (the byref object keeps the struct alive)
    return item


class DiscriminatorEngineCore(EngineBase):
    what = "discriminator"             # the reference class's name, for messages
    batch_stats = False                # BatchNorm layers: backward needs the batch statistics of a training-mode forward

    def __init__(self, owner: nn.Module, in_ch: int, sn_params: Sequence[str] = ()):
        """sn_params: names of the spectral-normalised weights (``....weight_orig``) in the order of their 1/sigma slots: layer l's
        sigma and 1/sigma are scalars[2l] and scalars[2l + 1] of the packed record, and every packed operand of the layer carries
        ``scale_off=2l + 1``"""
        super().__init__(owner, list(owner.named_parameters()))
        self.in_ch = in_ch
        # (parameter name, rows, cols) of the matrices torch's spectral_norm sees
        self.sn = [(n, p.shape[0], p[0].numel()) for n, p in ((n, self.fp.params[self.fp.index[n]]) for n in sn_params)]

    def _sn_uv(self, l: int) -> Tuple[Tensor, Tensor]:
        m = self.owner.get_submodule(self.sn[l][0].rsplit(".", 1)[0])
        return m.weight_u, m.weight_v

    # ---- packing: one power iteration per forward, then every operand is packed with 1/sigma of its layer multiplied in ----
    def _ensure_packed(self, dtc: int, device, training: bool) -> dict:
        pk = self._packed(dtc, device)
        flat = self.fp.flat
        if self.sn:
            if "scalars" not in pk:
                pk["scalars"] = torch.ones(2 * len(self.sn), dtype=torch.float32, device=device)
                pk["sn_ws"] = torch.empty(sum(A.sn_ws_floats(rows, cols) for _, rows, cols in self.sn), dtype=torch.float32, device=device)
            sc = pk["scalars"].data_ptr()
            layers = []
            for l, (name, rows, cols) in enumerate(self.sn):
                u, v = self._sn_uv(l)
                if u.device != flat.device or not u.is_contiguous() or not v.is_contiguous():
                    raise A.SrganfdError("spectral-norm buffers must live on the module's GPU")
                layers.append((flat.data_ptr() + 4 * self._poff(name), u.data_ptr(), v.data_ptr(), rows, cols, sc + 8 * l, sc + 8 * l + 4))
            ops.spectral_norm_batch(layers, training, pk["sn_ws"])            # all layers in four launches
        # the weights change every step and the power iteration moves sigma on every training forward: no staleness test
        pk["table"].run(flat, pk["buf"], pk.get("scalars"))
        return pk

    def _backward_workspaces(self, sp: _Shape, wplans: ops.WgradPlans, pk: dict) -> None:
        sp.wg_ws = wplans.workspace()
        # spectral-normalised layers write dL/d(W/sigma) here, each into its own range; passes with frozen parameters also send
        # BatchNorm's dgamma / dbeta here
        sp.gtmp = torch.zeros(self.fp.total, dtype=torch.float32, device=sp.device)
        sn_ws = torch.empty(len(self.sn) * A.SN_GRAD_WS_FLOATS, dtype=torch.float32, device=sp.device)
        sp.bw.append(SnGradBatch(self, [it.sn for it in sp.bw if isinstance(it, ops.Wgrad) and it.sn is not None], pk.get("scalars"), sn_ws))

    # ---- execution ----
    def _check_input(self, x: Tensor) -> None:
        check_channels(self.what, x, self.in_ch)

    def _logits(self, N: int, H: int, W: int, device) -> Tensor:
        return torch.empty(N, 1, H, W, dtype=torch.float32, device=device)

    def forward(self, x: Tensor, training: bool) -> Tensor:
        self._check_input(x)                       # the shape contract, before anything is packed, planned or launched
        _require_gpu(x)
        dt, dtc = _dt(self.owner)
        dev = x.device
        pk = self._ensure_packed(dtc, dev, training)
        N, _, H, W = x.shape
        sp = self._plan(N, H, W, dt, dtc, dev, pk)
        L, st = A.lib(), A.stream_ptr()
        x = x.contiguous().float()
        A.check(L.srganfd_nchw_to_nhwc(x.data_ptr(), N, self.in_ch, H, W, A.view(sp.xin), dtc, sp.xin.shape[-1], None, None, st), "nchw_to_nhwc")
        logits = self._logits(N, H, W, dev)
        ops.run_items(sp.fw, ops.Run("conv2d", training=training, out=logits.data_ptr()))
        self.token += 1
        sp.token, sp.training = self.token, training
        self._last = sp
        return logits

    def backward(self, sp: _Shape, token: int, dlogits: Tensor, need_wgrad: bool, need_dx: bool) -> Tuple[Optional[Tensor], Optional[Tensor]]:
        if getattr(sp, "token", None) != token:
            raise A.SrganfdError("discriminator activations / normalisation state were overwritten by a later forward before backward ran")
        if self.batch_stats and not sp.training:
            raise A.SrganfdError(f"{self.what} backward is implemented for training-mode forwards (BatchNorm batch statistics)")
        L, st = A.lib(), A.stream_ptr()
        N, H, W, dtc = sp.N, sp.H, sp.W, sp.dtc
        dlogits = dlogits.contiguous().float()
        A.check(L.srganfd_nchw_to_nhwc(dlogits.data_ptr(), N, 1, sp.dl.shape[1], sp.dl.shape[2], A.view(sp.dl), dtc, sp.dl.shape[-1], None, None, st),
                "nchw_to_nhwc")
        # frozen parameters: the weight-gradient launches are skipped; what else lands in the flat gradient goes to scratch
        flat_grad = self.fp.new_grad(sp.device) if need_wgrad else sp.gtmp
        run = ops.Run("conv2d(dgrad)", need_wgrad=need_wgrad, grad=flat_grad.data_ptr(), scratch=sp.gtmp.data_ptr(), ws=sp.wg_ws)
        ops.run_items(sp.bw, run)
        dx = None
        if need_dx:
            sp.dx_conv.launch(run)
            dx = torch.empty(N, self.in_ch, H, W, dtype=torch.float32, device=sp.device)
            A.check(L.srganfd_nhwc_to_nchw(A.view(sp.dxp), A.F32, N, self.in_ch, H, W, dx.data_ptr(), 0, st), "nhwc_to_nchw")
        return (flat_grad if need_wgrad else None), dx


class _DiscriminatorFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eng, training, *params):
        out = eng.forward(x, training)
        ctx.eng, ctx.sp, ctx.token = eng, eng._last, eng.token
        ctx.need_dx = ctx.needs_input_grad[0]
        ctx.need_w = any(ctx.needs_input_grad[3:])
        return out

    @staticmethod
    def backward(ctx, dlogits):
        g, dx = ctx.eng.backward(ctx.sp, ctx.token, dlogits, ctx.need_w, ctx.need_dx)
        grads = tuple(ctx.eng.fp.grad_views(g)) if g is not None else tuple(None for _ in ctx.eng.fp.params)
        return (dx, None, None) + grads


def discriminator_forward(eng: DiscriminatorEngineCore, owner: nn.Module, x: Tensor) -> Tensor:
    """the module's forward: through autograd when the input or a parameter wants a gradient"""
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in eng.fp.params)):
        return _DiscriminatorFn.apply(x, eng, owner.training, *eng.fp.params)
    return eng.forward(x, owner.training)
