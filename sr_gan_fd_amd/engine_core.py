"""What the three discriminator engines (engine_d.py, engine_a.py, engine_e.py) share: the spectral-norm state, the packing step
that runs its power iteration, the last item of their backward lists (SnGradBatch) and the plan data that is the same for all three.
The passes over the launch lists and the autograd glue are engine.py's (EngineBase).

A subclass describes its network: the layer tables, ``_build_pack``, ``_plan_forward`` / ``_plan_backward`` (the launch lists) and, beside
itself, the launch items only it has (BatchNorm).  Its plans always carry a backward list.  Of what EngineBase reads from a plan, a
subclass sets sp.xin (the NHWC input buffer: 4-channel pitch for the thin kernels, else padded to 32), sp.dl (NHWC buffer of the
logits' gradient), sp.dxp and sp.dx_conv (the fp32 NHWC4 gradient of the input and the item, ``first_layer_dgrad``, that writes it);
``_backward_workspaces`` derives the rest, sp.per_call among it: the shape of the logits, which the last forward item, an
ops.PerCall, writes.  In sp.bw, an ops.Wgrad carries ``sn``: the layer's spectral-norm slot, or None.
"""
from __future__ import annotations

import ctypes as C
import weakref
from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor, nn

from . import _abi as A
from . import ops
from .engine import EngineBase, _Shape


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
    out_ch = 1                         # the logits
    always_backward = True

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

    def _backward_workspaces(self, sp: _Shape, b: ops.PlanBuilder) -> None:
        """what every discriminator's plan ends with: where the passes enter and leave it (EngineBase), and the workspaces"""
        sp.x_in, sp.dy_in, sp.dx_out = (A.view(sp.xin), sp.xin.shape[-1]), (A.view(sp.dl), sp.dl.shape[-1]), (A.view(sp.dxp), A.F32)
        sp.hs, sp.ws = sp.dl.shape[1:3]
        sp.per_call = (sp.N, 1, sp.hs, sp.ws)
        sp.wg_ws = b.wplans.workspace()
        # spectral-normalised layers write dL/d(W/sigma) here, each into its own range; passes with frozen parameters also send
        # BatchNorm's dgamma / dbeta here
        sp.gtmp = torch.zeros(self.fp.total, dtype=torch.float32, device=sp.device)
        sn_ws = torch.empty(len(self.sn) * A.SN_GRAD_WS_FLOATS, dtype=torch.float32, device=sp.device)
        sp.bw.append(SnGradBatch(self, [it.sn for it in sp.bw if isinstance(it, ops.Wgrad) and it.sn is not None], b.pk.get("scalars"), sn_ws))

    def forward(self, x: Tensor, training: bool) -> Tensor:
        """the logits of one forward: always on a plan with a backward list, in the module's mode ``training``"""
        return self._pass(x, True, training)[1]
