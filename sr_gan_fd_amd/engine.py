"""Execution engines: sequence the HIP kernels (C ABI) for the reference's modules.

Host code here is plumbing only: it owns device buffers (torch tensors), builds the launch argument
structs once per input shape, and replays them on torch's current stream.  All arithmetic is in
libsrganfd_hip.so; nothing in this file falls back to PyTorch ops for compute.

Data layout in HBM (per engine, per input shape):
  * parameters: ONE flat fp32 buffer in ``named_parameters()`` order; every ``nn.Parameter`` of the
    module is re-pointed to a view of it (so optimizers / state_dict see the reference's tensors,
    while Adam, EMA and the gradient all-reduce work on one contiguous range).
  * packed weights: bf16 (or f32) MFMA B-fragment order, forward and data-gradient orientation,
    re-packed by one kernel launch whenever the flat parameter buffer changed.
  * activations: NHWC.  Each dense block owns ONE (N,H,W,C+4G) buffer: channels [0,C) are the
    block input, [C+kG, C+(k+1)G) the k-th growth conv's output -- torch.cat never runs, and the
    block's output is written by conv5's epilogue straight into the next block's channels [0,C).
  * backward: per dense block ONE stacked-gradient buffer [dOut(C) | dY4 | dY3 | dY2 | dY1]; the
    data-gradient of the block is again a dense block over that buffer (5 launches, no
    read-modify-write), and all five weight gradients come from one launch.
"""
from __future__ import annotations

import functools
import os
import weakref
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import Tensor, nn

from . import _abi as A
from . import ops

_ENGINES: "weakref.WeakKeyDictionary[nn.Module, object]" = weakref.WeakKeyDictionary()


def _require_gpu(x: Tensor) -> None:
    if not x.is_cuda and not A.DRY_RUN:
        raise A.SrganfdError("sr_gan_fd_amd runs on MI355X only: input tensor is not on a GPU (no CPU fallback)")
    A.lib()


def check_channels(what: str, x: Tensor, channels: int) -> None:
    """Host-side input contract of an image-side engine, checked before anything is planned, allocated or launched: a 4-D NCHW tensor
    with the channel count its first convolution reads (the boundary kernel reads N * channels * H * W elements of it)."""
    if x.dim() != 4 or x.shape[1] != channels:
        raise A.SrganfdError(f"{what} expects (N, {channels}, H, W) inputs, got shape {tuple(x.shape)}")


def resolve_compute_dtype(module) -> torch.dtype:
    """The reference's precision contract for its modules: a forward issued inside ``torch.autocast("cuda")`` (the training loops'
    ``amp.autocast()``, train_bsrgan.py:415-427,450-457; ESRGAN's validation too, train_rrdbnet.py:324-325) computes in the autocast
    dtype -- float16 by default, what the reference's convs run in on a GPU -- and one issued outside it (``validate()``,
    train_bsrgan.py:563; inference.py:60-70) in float32.  ``module.compute_dtype`` (None by default) overrides both.  The backward
    pass always runs in the dtype of the forward whose activations it consumes (the plan's), as autograd does under autocast."""
    dt = getattr(module, "compute_dtype", None)
    if dt is not None:
        return dt
    if torch.is_autocast_enabled("cuda"):
        return torch.get_autocast_dtype("cuda")
    return torch.float32


def _dt(module) -> Tuple[torch.dtype, int]:
    dt = resolve_compute_dtype(module)
    if dt not in ops.DT:
        raise A.SrganfdError(f"compute dtype {dt} is not supported (float32, float16, bfloat16)")
    return dt, ops.DT[dt]


# ------------------------------------------------------------------------------------------------
# flat parameter storage
# ------------------------------------------------------------------------------------------------
class FlatParams:
    """Keeps a module's parameters as views of one contiguous fp32 buffer."""

    def __init__(self, named: Sequence[Tuple[str, nn.Parameter]]):
        self.names = [n for n, _ in named]
        self.params = [p for _, p in named]
        self.shapes = [tuple(p.shape) for p in self.params]
        self.numels = [p.numel() for p in self.params]
        self.offsets, off = [], 0
        for n in self.numels:
            self.offsets.append(off)
            off += (n + 3) // 4 * 4          # keep every tensor 16-byte aligned
        self.total = off
        self.index = {n: i for i, n in enumerate(self.names)}
        self.flat: Optional[Tensor] = None
        self.version = 0                       # bumped by whoever writes the flat buffer behind autograd's back (touch())
        self.unwritten = False                 # True: some parameter's range of the flat gradient is written by no launch (new_grad zeroes)

    def off(self, name: str) -> int:
        return self.offsets[self.index[name]]

    def sync(self, device) -> Tensor:
        """(Re)build the flat buffer if any parameter moved (``.to()``, deepcopy, fresh module)."""
        f = self.flat
        ok = f is not None and f.device == device
        if ok:
            base = f.data_ptr()
            for p, o in zip(self.params, self.offsets):
                if p.data_ptr() != base + 4 * o:
                    ok = False
                    break
        if not ok:
            f = torch.zeros(self.total, dtype=torch.float32, device=device)
            with torch.no_grad():
                for p, o, n, s in zip(self.params, self.offsets, self.numels, self.shapes):
                    f[o:o + n].copy_(p.detach().reshape(-1).to(device=device, dtype=torch.float32))
                    p.data = f[o:o + n].view(s)
            self.flat = f
            self.version += 1
        return f

    def touch(self) -> None:
        """The flat buffer was written by a kernel (fused Adam): every packed copy, of every compute dtype, is stale."""
        self.version += 1

    def signature(self) -> tuple:
        """Identity of the current parameter VALUES (tensor version counters + touch() count)."""
        return (self.flat.data_ptr(), self.flat._version, self.version, tuple(p._version for p in self.params))

    def stale(self, pk: dict) -> bool:
        """True if the packed-weight record `pk` (one per compute dtype) was packed from other values; marks it fresh.
        The signature is kept PER PACK: with one shared marker, the first forward in dtype A after an optimizer step consumed the
        change and a following forward in dtype B ran on weights from before the step."""
        sig = self.signature()
        if pk.get("seen") != sig:
            pk["seen"] = sig
            return True
        return False

    def new_grad(self, device) -> Tensor:
        """Flat gradient buffer.  Tensors whose size is not a multiple of 4 leave alignment gaps that no kernel writes: zero
        them (the optimizer walks the whole buffer), otherwise the gaps of the parameter buffer pick up allocator garbage and
        two identical runs stop being bitwise equal (found by tests/test_fullsize_gpu.py)."""
        if self.total == sum(self.numels) and not self.unwritten:
            return torch.empty(self.total, dtype=torch.float32, device=device)
        return torch.zeros(self.total, dtype=torch.float32, device=device)

    def grad_views(self, flat_grad: Tensor) -> List[Tensor]:
        return [flat_grad[o:o + n].view(s) for o, n, s in zip(self.offsets, self.numels, self.shapes)]


# ------------------------------------------------------------------------------------------------
# generator (RRDBNet / BSRGAN) engine
# ------------------------------------------------------------------------------------------------
class _Shape:
    """Per-(N,H,W,training) buffers and pre-built launch lists.  EngineBase names what the passes read of a plan; the class
    attributes are what a plan that has no such thing need not set."""
    result = per_call = dx_out = dx_conv = gtmp = token = None


class PlanCache:
    """Per-shape plans, least-recently-used eviction.  Training plans are pinned (at most two are kept): a validation sweep over
    many image sizes (inference.py / validate()) evicts only other inference plans, never the multi-GB training
    plan of the step it runs between -- the earlier `clear()` on overflow dropped everything."""

    def __init__(self, cap: int = 8, cap_pinned: int = 2):
        from collections import OrderedDict
        self.d: "OrderedDict[tuple, tuple]" = OrderedDict()
        self.cap, self.cap_pinned = cap, cap_pinned

    def get(self, key):
        v = self.d.get(key)
        if v is None:
            return None
        self.d.move_to_end(key)
        return v[0]

    def put(self, key, sp, pinned: bool = False) -> None:
        self.d[key] = (sp, pinned)
        self.d.move_to_end(key)
        for want_pinned, cap in ((False, self.cap), (True, self.cap_pinned)):
            keys = [k for k, (_, pin) in self.d.items() if pin == want_pinned]
            for k in keys[:max(0, len(keys) - cap)]:
                del self.d[k]

    def __setitem__(self, key, sp) -> None:
        self.put(key, sp)

    def __len__(self) -> int:
        return len(self.d)

    def __contains__(self, key) -> bool:
        return key in self.d

    def clear(self) -> None:
        self.d.clear()


class EngineBase:
    """What every engine owns: the module's parameters as one flat buffer, the per-shape plans, one packed-weight record per compute
    dtype (built by the subclass's ``_build_pack``), the token that ties a backward pass to its forward, and the one forward and
    backward pass over a plan's launch lists.

    A subclass describes its network -- ``_build_pack`` and the two halves of a plan, ``_plan_forward(sp, b, train)`` and
    ``_plan_backward(sp, b)`` (``b``: the plan's ops.PlanBuilder), which ``_plan`` calls for a shape it has no plan for yet -- and
    names its ``what`` (the reference class, for messages), ``in_ch`` and ``out_ch``.  What differs between the engines at the boundary of a
    pass is data on the plan ``sp`` (items: ops.py's, each with ``launch(run)``):
      sp.fw                  forward items
      sp.x_in                (view, pitch): where the NCHW input goes as NHWC, in_ch real channels of ``pitch`` written
      sp.hs, sp.ws           height and width of the result
      sp.result              (view, dtype code, clamp): the NHWC buffer the (N, out_ch, hs, ws) result is read from (``clamp``: to
                             [0, 1], the generator's image), or None: the result is the per-call tensor
      sp.per_call            shape of an fp32 tensor allocated per forward, which the list's ops.PerCall item writes (``run.out``): the
                             discriminators' logits, SelfAttention's weights; or None
    and, on a plan built with ``train`` (sp.token: the forward it holds the activations of),
      sp.bw                  backward items
      sp.dy_in               (view, pitch): where the result's NCHW gradient goes as NHWC (through the clamp's derivative where the
                             result was clamped)
      sp.dx_out              (view, dtype code) of the input's gradient, or None (an image: nobody asks)
      sp.dx_conv             None, or the item of the first layer's data gradient: launched only by a pass that wants dx
      sp.wg_ws, sp.gtmp      the weight-gradient workspace; None, or the scratch gradient of an engine whose backward list writes
                             gradients that are no Wgrad's (BatchNorm, spectral norm): where they go when the parameters are frozen"""
    what = "engine"
    unshuffle = 1                      # PixelUnshuffle factor in front of the first layer (Real-ESRGAN's generator below x4)
    batch_stats = False                # BatchNorm layers: backward needs the batch statistics of a training-mode forward
    always_backward = False            # True: every plan carries a backward list, is not keyed on ``train`` and is never pinned
    conv_batch = None                  # the batch of the plan's conv launches where it is not the plan's N (ops.PlanBuilder's ``n``)

    def __init__(self, owner: nn.Module, named_params: Sequence[Tuple[str, nn.Parameter]]):
        self.owner = owner
        self.fp = FlatParams(named_params)
        self.shapes = PlanCache()
        self.packed: Dict[int, dict] = {}
        self.token = 0

    def _poff(self, name: str) -> int:
        return self.fp.off(name)

    def _packed(self, dtc: int, device) -> dict:
        """the packed-weight record of a dtype, rebuilt when the parameters moved to another device or flat buffer"""
        flat = self.fp.sync(device)
        pk = self.packed.get(dtc)
        if pk is None or pk["buf"].device != device or pk.get("flat_ptr") != flat.data_ptr():
            pk = self._build_pack(dtc, device)
            pk["flat_ptr"] = flat.data_ptr()
            self.packed[dtc] = pk
        return pk

    def _ensure_packed(self, dtc: int, device, training: bool = False) -> dict:
        """... and packed again when the parameter values changed since this record was last packed"""
        pk = self._packed(dtc, device)
        if self.fp.stale(pk):
            pk["table"].run(self.fp.flat, pk["buf"])
        return pk

    # -- per-shape plan -----------------------------------------------------------------------
    def _plan_key(self) -> tuple:
        """what a plan depends on besides shape, dtype, buffers and ``train``"""
        return ()

    def _plan(self, N: int, H: int, W: int, dt: torch.dtype, dtc: int, device, pk: dict, train: bool) -> _Shape:
        train = train or self.always_backward
        # the launch lists bake absolute pointers into the packed buffer AND the flat parameter buffer (biases): both are in the key
        key = (N, H, W, dtc) + (() if self.always_backward else (train,)) + (str(device), pk["buf"].data_ptr(), self.fp.flat.data_ptr()) + self._plan_key()
        sp = self.shapes.get(key)
        if sp is None:
            sp = _Shape()
            sp.N, sp.H, sp.W, sp.dt, sp.dtc, sp.device = N, H, W, dt, dtc, device
            b = ops.PlanBuilder(self, sp, pk, n=self.conv_batch)
            self._plan_forward(sp, b, train)
            if train:
                self._plan_backward(sp, b)
            self.shapes.put(key, sp, pinned=train and not self.always_backward)
        return sp

    # -- execution ----------------------------------------------------------------------------
    def _check_input(self, x: Tensor) -> Tuple[int, int, int]:
        """the input contract, checked before anything is packed, planned or launched; returns the (N, H, W) the plan is built for"""
        check_channels(self.what, x, self.in_ch)
        return x.shape[0], x.shape[2], x.shape[3]

    def _pass(self, x: Tensor, train: bool, training: bool = False, per_call: bool = True) -> Tuple[Optional[Tensor], Optional[Tensor]]:
        """One forward pass.  x: NCHW; ``train``: on a plan with a backward list, which then holds this pass's activations;
        ``training``: the module's mode (BatchNorm statistics, spectral-norm iteration); ``per_call``: False skips the plan's per-call
        tensor and the launch that writes it.  Returns (the NCHW fp32 result read from sp.result, the per-call tensor)."""
        N, H, W = self._check_input(x)
        _require_gpu(x)
        dt, dtc = _dt(self.owner)
        dev = x.device
        pk = self._ensure_packed(dtc, dev, training)
        sp = self._plan(N, H, W, dt, dtc, dev, pk, train)
        if self.unshuffle > 1:
            # a pure re-indexing of the image (no parameters, no arithmetic; the image needs no gradient): conv1 then reads 12 / 48
            # channels (padded to 32 / 64 for the MFMA path) at the trunk's size
            x = torch.nn.functional.pixel_unshuffle(x, self.unshuffle)
        x = x.contiguous().float()
        L, st = A.lib(), A.stream_ptr()
        view, pitch = sp.x_in
        A.check(L.srganfd_nchw_to_nhwc(x.data_ptr(), N, self.in_ch, H, W, view, dtc, pitch, None, None, st), "nchw_to_nhwc")
        own = torch.empty(sp.per_call, dtype=torch.float32, device=dev) if per_call and sp.per_call else None
        ops.run_items(sp.fw, ops.Run("conv2d", training=training, out=0 if own is None else own.data_ptr()))
        out = None
        if sp.result is not None:
            view, code, clamp = sp.result
            out = torch.empty(N, self.out_ch, sp.hs, sp.ws, dtype=torch.float32, device=dev)
            A.check(L.srganfd_nhwc_to_nchw(view, code, N, self.out_ch, sp.hs, sp.ws, out.data_ptr(), clamp, st), "nhwc_to_nchw")
        if train:
            self.token += 1
            sp.token, sp.training = self.token, training
        self._last = sp
        return out, own

    def forward(self, x: Tensor, train: bool) -> Tensor:
        """x: NCHW (an image, or a lone block's feature map).  Returns NCHW fp32."""
        return self._pass(x, train)[0]

    def backward(self, sp: "_Shape", token: int, dout: Tensor, need_wgrad: bool, need_dx: bool, on_ready=None) -> Tuple[Optional[Tensor], Optional[Tensor]]:
        """dout: NCHW gradient of forward()'s result.  Returns (flat parameter gradient or None, dx or None); a pass with frozen
        parameters (``need_wgrad`` False) skips the weight-gradient launches.  ``on_ready(flat_grad, lo, hi)`` (data parallelism,
        parallel.BucketReducer.bucket) is called when every launch that writes elements [lo, hi) of the flat gradient has been
        enqueued; the ranges are disjoint and cover the whole buffer."""
        if sp.token != token:
            raise A.SrganfdError(f"{self.what}: activations or normalisation state were overwritten by a later forward of the same module "
                                 "before backward ran")
        if self.batch_stats and not sp.training:
            raise A.SrganfdError(f"{self.what} backward is implemented for training-mode forwards (BatchNorm batch statistics)")
        L, st = A.lib(), A.stream_ptr()
        N, dtc = sp.N, sp.dtc
        dout = dout.contiguous().float()
        view, pitch = sp.dy_in
        if sp.result is not None and sp.result[2]:
            A.check(L.srganfd_clamp_grad_to_nhwc(dout.data_ptr(), sp.result[0], N, self.out_ch, sp.hs, sp.ws, view, dtc, pitch, st), "clamp_grad")
        else:
            A.check(L.srganfd_nchw_to_nhwc(dout.data_ptr(), N, self.out_ch, sp.hs, sp.ws, view, dtc, pitch, None, None, st), "nchw_to_nhwc")
        # frozen parameters: what else lands in the flat gradient goes to the scratch gradient
        flat_grad = self.fp.new_grad(sp.device) if need_wgrad else sp.gtmp
        run = ops.Run("conv2d(dgrad)", need_wgrad=need_wgrad, grad=0 if flat_grad is None else flat_grad.data_ptr(),
                      scratch=0 if sp.gtmp is None else sp.gtmp.data_ptr(), ws=sp.wg_ws,
                      on_ready=None if on_ready is None else functools.partial(on_ready, flat_grad))
        ops.run_items(sp.bw, run)
        dx = None
        if need_dx and sp.dx_out is not None:
            if sp.dx_conv is not None:
                sp.dx_conv.launch(run)
            view, code = sp.dx_out
            dx = torch.empty(N, self.in_ch, sp.H, sp.W, dtype=torch.float32, device=sp.device)
            A.check(L.srganfd_nhwc_to_nchw(view, code, N, self.in_ch, sp.H, sp.W, dx.data_ptr(), 0, st), "nhwc_to_nchw")
        return (flat_grad if need_wgrad else None), dx


class TrunkEngine(EngineBase):
    """Forward/backward of a chain of residual dense blocks, optionally wrapped by the generator's
    head (conv1) and tail (conv2, upsampling, conv3, conv4, clamp).

    Reference: _ResidualDenseBlock.forward BSRGAN/model.py:51-62, _ResidualResidualDenseBlock.forward
    :79-88, BSRGAN._forward_impl :366-381 (RRDBNet: ESRGAN/model.py:208-229)."""

    def __init__(self, owner: nn.Module, rdbs: Sequence[nn.Module], rrdb: bool, full: bool):
        super().__init__(owner, list(owner.named_parameters()))
        self.rdbs = list(rdbs)
        self.rrdb = rrdb
        self.full = full
        self.R = len(self.rdbs)
        c5 = self.rdbs[0].conv5.weight
        self.Cc = c5.shape[0]                       # channels
        self.G = self.rdbs[0].conv1.weight.shape[0]  # growth channels
        if self.Cc % 32 or self.G % 32:
            raise A.SrganfdError("channels and growth_channels must be multiples of 32 for the MFMA path")
        self.Ccat = self.Cc + 4 * self.G
        self.what = "generator" if full else "dense block"
        self.in_ch = self.out_ch = self.Cc
        # nearest-x2 + 3x3 upsampling layers in parity form (16-bit modes): the forward as four 2x2-tap classes over the low-res input, the data
        # gradient as one 4x4 stride-2 conv over the high-res gradient.  0: the up=1 gather forward, the high-res data gradient and the
        # nearest adjoint (same-process A/B: the switch is read when the engine is built)
        self.up_parity = os.environ.get("SRGANFD_UPSAMPLE_PARITY", "1") != "0"
        if full:
            self.n_up = owner.n_upsample()
            self.in_ch = owner.conv1.weight.shape[1]
            self.out_ch = owner.conv4.weight.shape[0]
            # Real-ESRGAN below x4 (Real_ESRGAN/model.py:190-204,248): PixelUnshuffle(2 / 4) in front of conv1, applied in forward() so
            # that the module path and the fused trainers share it
            self.unshuffle = getattr(owner, "unshuffle", 1)
        self._rdb_prefix = self._find_prefixes()

    # -- parameter bookkeeping ----------------------------------------------------------------
    def _find_prefixes(self) -> List[str]:
        names = {id(m): n for n, m in self.owner.named_modules()}
        out = []
        for r in self.rdbs:
            n = names[id(r)]
            out.append(n + "." if n else "")
        return out

    def _parity(self, dtc: int) -> bool:
        """do the upsampling layers run in parity form?  (16-bit modes: the class launch has no fp32 kernel)"""
        return self.full and self.up_parity and dtc != A.F32

    def _build_pack(self, dtc: int, device) -> dict:
        """Pack-job tables + offsets of every packed operand (forward and data-gradient)."""
        Cc, G, Ccat = self.Cc, self.G, self.Ccat
        pb = ops.PackBuilder(dtc)
        fwd = lambda key, wname, co, ci: pb.fwd(key, self._poff(wname), co, ci)
        bwd = lambda key, wname, co, ci: pb.bwd(key, self._poff(wname), co, ci)

        for i, pre in enumerate(self._rdb_prefix):
            for k in range(1, 6):
                cin, cout = Cc + (k - 1) * G, (Cc if k == 5 else G)
                fwd(("f", i, k), f"{pre}conv{k}.weight", cout, cin)
            # data gradient of the block = dense block over [dOut(C) | dY4 | dY3 | dY2 | dY1]
            s5 = 0.2 * (0.2 if (self.rrdb and i % 3 == 2) else 1.0)
            dyoff = {5: 0, 4: Cc, 3: Cc + G, 2: Cc + 2 * G, 1: Cc + 3 * G}
            for step in range(5):               # step 0..3 -> dY4..dY1, step 4 -> dX
                c_lo = Cc + (3 - step) * G if step < 4 else 0
                n = G if step < 4 else Cc
                kdim = Cc + step * G
                segs = []
                for j in range(5, 4 - step, -1):   # convs whose input covers channels [c_lo, c_lo+n)
                    cin_j, cout_j = Cc + (j - 1) * G, (Cc if j == 5 else G)
                    segs.append(dict(src_off=self._poff(f"{pre}conv{j}.weight"), co_src=cout_j, ci_src=cin_j, k_lo=dyoff[j],
                                     k_len=cout_j, ci_off=c_lo, transposed=1, scale=(s5 if j == 5 else 1.0)))
                pb.add(("b", i, step), 3, kdim, n, segs)
        if self.full:
            fwd(("f", "conv1"), "conv1.weight", Cc, self.in_ch)
            self._stage_pack(pb, dtc)
            ups = [f"upsampling{u}.0" for u in range(1, self.n_up + 1)]
            for nm in ["conv2"] + ups + ["conv3.0"]:
                if nm in ups and self._parity(dtc):
                    # forward: four 2x2-tap class operands back to back (pack codes 14..17); data gradient: one 4x4 operand (code 18)
                    pb.classes(("fc", nm), self._poff(nm + ".weight"), Cc, Cc, 2, 14)
                    pb.bwd(("b4", nm), self._poff(nm + ".weight"), Cc, Cc, 4, transposed=18)
                    continue
                fwd(("f", nm), nm + ".weight", Cc, Cc)
                bwd(("b", nm), nm + ".weight", Cc, Cc)
            fwd(("f", "conv4"), "conv4.weight", self.out_ch, Cc)
            bwd(("b", "conv4"), "conv4.weight", self.out_ch, Cc)
        return pb.finish(device)

    # -- per-shape plan -----------------------------------------------------------------------
    def _plan_forward(self, sp: _Shape, b: ops.PlanBuilder, train: bool) -> None:
        N, H, W, dtc = sp.N, sp.H, sp.W, sp.dtc
        Cc, G, Ccat, R = self.Cc, self.G, self.Ccat, self.R
        if train:
            cat = sp.cat = [b.act(H, W, Ccat) for _ in range(R + 1)]
            catb = lambda i: cat[i]            # (captures the list, not `sp`: a closure stored on sp that refers to sp is a cycle)
        else:
            # inference: block 0's buffer is kept (conv2 adds out1, model.py:369-370); the rest rotate.
            # block i reads buffer i, writes i+1, and (last block of an RRDB) re-reads i-2: 4 buffers suffice.
            cat = sp.cat = [b.act(H, W, Ccat) for _ in range(min(R + 1, 5))]
            catb = lambda i: cat[0] if i == 0 else cat[1 + (i - 1) % 4]
        sp.catb = catb
        V = A.view
        # the dense-block buffers of the full generator are stored as planar 32-channel groups (srganfd_view.planar): every
        # 32-channel chunk pass of a conv / weight-gradient launch then reads whole contiguous lines instead of 64 of the 384 bytes
        # of each pixel, and the 96- / 160-channel convs stop fetching half-used lines.  Stand-alone blocks keep NHWC (their
        # boundary kernels convert NCHW <-> NHWC directly into / out of these buffers).
        sp.planar = 1 if (self.full and os.environ.get("SRGANFD_PLANAR", "1") != "0") else 0
        VC = lambda t, c0=0: A.view(t, c0=c0, planar=sp.planar)
        lre = dict(act=A.ACT_LRELU, slope=0.2)

        fw = []   # forward launch list
        if self.full:
            s = 1 << self.n_up
            # thin-side kernels (csrc/conv_thin.hip) for conv1 / conv4 in the 16-bit modes: the image side is NHWC with a 4-channel pitch
            sp.thin_i, sp.thin_o = ops.thin_ok(dtc, Cc, self.in_ch), ops.thin_ok(dtc, Cc, self.out_ch)
            cin1 = ops.pad32(self.in_ch)          # 3 -> 32; Real-ESRGAN below x4: 12 -> 32, 48 -> 64 (Real_ESRGAN/model.py:190-201)
            sp.xin = b.act(H, W, 4 if sp.thin_i else cin1)
            sp.f0 = b.act(H, W, Cc)
            sp.ups = [b.act(H << u, W << u, Cc) for u in range(1, self.n_up + 1)]
            sp.c3 = b.act(H * s, W * s, Cc)
            sp.srp = b.act(H * s, W * s, 4, dtype=torch.float32)
            fw.append(b.image_to_features(sp.thin_i, sp.xin, VC(catb(0)), "conv1", H, W, self.in_ch, Cc, True))
        for i, pre in enumerate(self._rdb_prefix):
            ci = catb(i)
            blk = []
            for k in range(1, 5):
                blk.append(ops.conv_args(dtc, VC(ci), VC(ci, c0=Cc + (k - 1) * G), b.Wp(("f", i, k)), N, H, W, Cc + (k - 1) * G, G,
                                         bias=b.P(f"{pre}conv{k}.bias"), **lre))
            last = self.rrdb and i % 3 == 2
            kw = dict(post_scale=0.04, r1=VC(ci), r1_scale=0.2, r2=VC(catb(i - 2)), r2_scale=1.0) if last else \
                dict(post_scale=0.2, r1=VC(ci), r1_scale=1.0)
            blk.append(ops.conv_args(dtc, VC(ci), VC(catb(i + 1)), b.Wp(("f", i, 5)), N, H, W, Ccat, Cc, bias=b.P(f"{pre}conv5.bias"), **kw))
            # small batches (the reference's own crop sizes): the five launches as ONE LDS-resident launch (csrc/dense_chain.hip)
            fw.extend(ops.dense_chain_or_launches(blk, sp.device) if (Cc, G) == (64, 32) else [ops.Conv(a) for a in blk])
        if self.full:
            # what conv2 reads: the trunk's output, or the output of a stage between the two (BSRGANtrans, engine_trans.py)
            sp.conv2_in = self._stage_forward(sp, b, fw, VC(catb(R)), train)
            fw.append(b.conv(sp.conv2_in, sp.f0, ("f", "conv2"), H, W, Cc, Cc, bias=b.P("conv2.bias"), r1=VC(catb(0)), r1_scale=1.0))
            src, h, w = sp.f0, H, W
            for u in range(1, self.n_up + 1):
                nm = f"upsampling{u}.0"
                if self._parity(dtc):
                    fw.extend(self._up_forward(b, V(src), V(sp.ups[u - 1]), h, w, nm))
                else:
                    fw.append(b.conv(src, sp.ups[u - 1], ("f", nm), h, w, Cc, Cc, up=1, bias=b.P(nm + ".bias"), **lre))
                src, h, w = sp.ups[u - 1], h * 2, w * 2
            fw.append(b.conv(src, sp.c3, ("f", "conv3.0"), h, w, Cc, Cc, bias=b.P("conv3.0.bias"), **lre))
            fw.append(b.features_to_image(sp.thin_o, sp.c3, sp.srp, 4, "conv4", h, w, self.out_ch, Cc, False))
            sp.hs, sp.ws = h, w
            sp.x_in, sp.result = (V(sp.xin), sp.xin.shape[-1]), (V(sp.srp), A.F32, 1)
        else:
            sp.hs, sp.ws = H, W
            sp.x_in, sp.result = (V(catb(0)), Cc), (V(catb(R)), dtc, 0)
        sp.fw = fw

    def _up_forward(self, b: ops.PlanBuilder, x: A.View, y: A.View, h: int, w: int, nm: str) -> List[ops.Conv]:
        """nearest x2 + 3x3 pad-1 conv + LeakyReLU (BSRGAN/model.py:372-374) as its four output-parity classes: 2x2-tap convs over the
        low-res input x (pack codes 14..17), written into the high-res y.  One launch when the library takes the four classes together
        (ops.class4_ok), else one launch per class."""
        Cc = self.Cc
        return ops.parity_class_launches(b.dtc, x, y, b.wptr, [b.offs[("fc", nm, c)] for c in range(4)], b.N, h, w, Cc, Cc, 2, 1,
                                         tag=" nearest-x2 fwd", bias=b.P(nm + ".bias"), act=A.ACT_LRELU, slope=0.2)      # class (py, px) reads the window at (oy + py - 1, ox + px - 1)

    def _block_s5(self, i: int) -> float:
        """the scale of block i's conv5 output: 0.2, times the RRDB's 0.2 in its last block"""
        return 0.2 * (0.2 if (self.rrdb and i % 3 == 2) else 1.0)

    def _dense_plan(self, sp: _Shape, b: ops.PlanBuilder, s5: float, splits: int = 0) -> ops.WgradPlan:
        """a dense block's weight-gradient plan, by (conv5's scale, pixel splits; 0: the library's choice for one block per launch)"""
        if (s5, splits) not in sp.dense_plans:
            Cc, G, Ccat = self.Cc, self.G, self.Ccat
            convs, pre = [], self._rdb_prefix[0]            # the plan's offsets are relative to the block: every block's are block 0's
            rel = self._poff(pre + "conv1.weight")
            for k in range(1, 6):
                cin, cout = Cc + (k - 1) * G, (Cc if k == 5 else G)
                convs.append(dict(ci_lo=0, cin=cin, co_lo=(0 if k == 5 else Cc + (4 - k) * G), cout=cout,
                                  dw_off=self._poff(pre + f"conv{k}.weight") - rel, db_off=self._poff(pre + f"conv{k}.bias") - rel,
                                  co_dst=cout, ci_dst=cin, alpha=(s5 if k == 5 else 1.0)))
            sp.dense_plans[(s5, splits)] = b.wplans.plan(sp.H, sp.W, Ccat, Ccat, convs, splits=splits)
        return sp.dense_plans[(s5, splits)]

    def _plan_backward(self, sp: _Shape, b: ops.PlanBuilder) -> None:
        N, H, W, dtc = sp.N, sp.H, sp.W, sp.dtc
        Cc, G, Ccat, R = self.Cc, self.G, self.Ccat, self.R
        V = A.view
        VD = lambda t, c0=0: A.view(t, c0=c0, planar=sp.planar)      # the stacked-gradient buffers: the layout of the forward's dense-block buffers
        #                                                              (planar only one of the two measured half the gain each)
        sp.dense_plans = {}
        # _BATCH_WGRAD: up to _BATCH_REDUCE blocks' weight gradients as one MFMA launch (batch_wgrads).  "auto": where one block's
        # launch already fills the chip -- at least as many pixel tiles as the device gives it splits -- so that a batch's fewer
        # splits per block lose nothing
        p0 = self._dense_plan(sp, b, self._block_s5(R - 1))
        sp.batch_wgrad = _BATCH_REDUCE > 1 and (_BATCH_WGRAD == "1" or (_BATCH_WGRAD == "auto" and p0.ntiles >= max(1, ops.device_cus(sp.device) // p0.ngroups)))
        # a batch's launch stands at its LAST block and reads every block's stacked-gradient buffer there.  Per-layer data gradients:
        # four rotating buffers hold that long (a block's 192->64 launch, which overwrites the buffer four blocks up, follows its weight
        # gradient; a batch of more than four blocks needs one each).  The dense-block launch takes all five convs before it: one
        # buffer more than a batch has blocks
        chain_form = (Cc, G) == (64, 32) and dtc in (A.F16, A.BF16) and ops.dense_chain_wanted(N, H, W)
        ndy = max(4, _BATCH_REDUCE + (1 if chain_form else 0)) if sp.batch_wgrad else 4
        sp.dy = [b.act(H, W, Ccat) for _ in range(ndy)]
        sp.dx0 = b.act(H, W, Cc)            # gradient w.r.t. the trunk input
        dyb = lambda i: sp.dy[i % ndy]
        if not self.full:
            sp.dy_in, sp.dx_out = (V(dyb(R - 1)), Cc), (V(sp.dx0), dtc)
        # ops.Conv | Wgrad | ThinLaunch | DenseChain | Call and the bucket markers ops.Ready
        bw = self._backward_tail(sp, b, VD(dyb(R - 1))) if self.full else []
        bw += self._backward_blocks(sp, b, dyb, VD)
        if self.full:
            bw.append(ops.Call("srganfd_axpby", (V(sp.d_f0), V(sp.dx0), dtc, N * H * W, Cc, 1.0, 1.0), "axpby"))
            bw.append(b.image_wgrad(sp.thin_i, sp.xin, sp.dx0, "conv1", sp.thin_ws, H, W, self.in_ch, Cc, True))
        # last bucket: whatever the earlier markers did not cover
        covered = min([it.lo for it in bw if isinstance(it, ops.Ready)], default=self.fp.total)
        bw.append(ops.Ready(0, covered))
        self._finish_backward(sp, b)
        sp.wg_ws = b.wplans.workspace()
        sp.bw = self._batch_dense_wgrads(sp, b, bw, p0)

    def _backward_tail(self, sp: _Shape, b: ops.PlanBuilder, trunk_grad: A.View) -> list:
        """the generator's tail, from the image's gradient to ``trunk_grad`` (channels [0, Cc) of the last dense block's stacked-gradient
        buffer): conv4, conv3, the upsampling stages, conv2, the first gradient bucket and the stage between trunk and conv2"""
        N, H, W, dtc, Cc, V = sp.N, sp.H, sp.W, sp.dtc, self.Cc, A.view
        hs, ws_ = sp.hs, sp.ws
        sp.dsrp = b.act(hs, ws_, 4 if sp.thin_o else 32)
        sp.dy_in = (V(sp.dsrp), sp.dsrp.shape[-1])
        sp.gA, sp.gB = b.act(hs, ws_, Cc), b.act(hs, ws_, Cc)
        sp.thin_ws = b.thin_ws(sp.thin_i, sp.thin_o)
        sp.glo = [b.act(H << u, W << u, Cc) for u in range(0, self.n_up)]   # grads at the input res of upsampling u+1
        src3 = sp.ups[-1] if self.n_up else sp.f0
        bw = [
            b.image_wgrad(sp.thin_o, sp.dsrp, sp.c3, "conv4", sp.thin_ws, hs, ws_, self.out_ch, Cc, False),
            b.image_to_features(sp.thin_o, sp.dsrp, sp.gA, "conv4", hs, ws_, self.out_ch, Cc, False, flip=True, mask=V(sp.c3), mask_slope=0.2),
            b.wgrad(src3, sp.gA, hs, ws_, Cc, Cc, "conv3.0.weight", "conv3.0.bias"),
            b.dgrad(sp.gA, sp.gB, ("b", "conv3.0"), hs, ws_, Cc, Cc, mask=src3 if self.n_up else None),
        ]
        cur, other = sp.gB, sp.gA        # cur = gradient w.r.t. pre-activation of upsampling{n_up} (at its output res)
        for u in range(self.n_up, 0, -1):
            nm = f"upsampling{u}.0"
            hin, win = H << (u - 1), W << (u - 1)
            xin_t = sp.ups[u - 2] if u >= 2 else sp.f0
            npx = N * (hin * 2) * (win * 2)
            cur_v = V(cur.view(-1)[: npx * Cc].view(N, hin * 2, win * 2, Cc))
            oth_v = V(other.view(-1)[: npx * Cc].view(N, hin * 2, win * 2, Cc))
            bw.append(b.wgrad(xin_t, cur_v, hin, win, Cc, Cc, nm + ".weight", nm + ".bias", up=1))
            glo = sp.glo[u - 1]
            if self._parity(dtc):
                # data gradient, nearest adjoint and (u >= 2: the input is the previous upsampling conv's LeakyReLU output) LeakyReLU' as
                # ONE 4x4 stride-2 pad-1 conv over the high-res gradient, written at the low resolution
                it = b.dgrad(cur_v, glo, ("b4", nm), hin * 2, win * 2, Cc, Cc, mask=xin_t if u >= 2 else None, ksize=4, stride=2, pad=1)
                it.args._label_tag = " nearest-x2 dgrad"
                bw.append(it)
            else:
                bw.append(b.dgrad(cur_v, oth_v, ("b", nm), hin * 2, win * 2, Cc, Cc))
                bw.append(b.resample(0, oth_v, glo, hin, win, Cc, what="nearest_bwd"))
                if u >= 2:   # input of this stage is the LeakyReLU output of the previous upsampling conv
                    bw.append(b.lrelu_bwd(glo, xin_t, glo, N * hin * win, Cc))
            cur, other = glo, sp.gA      # the next stage works at (hin, win): gA is its scratch, the gradient lives in glo
        d_f0 = sp.d_f0 = cur if self.n_up else sp.gB
        # conv2: f0 = out1 + conv2(trunk_out)
        bw.append(b.wgrad(sp.conv2_in, d_f0, H, W, Cc, Cc, "conv2.weight", "conv2.bias"))
        dst2, epi2 = self._conv2_dgrad_target(sp, trunk_grad)
        bw.append(b.conv(d_f0, dst2, ("b", "conv2"), H, W, Cc, Cc, **epi2))
        # gradient buckets for the data-parallel exchange (parallel.BucketReducer): parameters sit in named_parameters() order --
        # conv1, the dense blocks, conv2 and the tail -- so "everything from conv2 on" is one contiguous range, final here
        bw.append(ops.Ready(self._poff("conv2.weight"), self.fp.total))
        # a stage between trunk and conv2: its backward ends in the last dense block's stacked-gradient buffer, its parameters are final
        bw.extend(self._stage_backward(sp, b, trunk_grad))
        return bw

    def _backward_blocks(self, sp: _Shape, b: ops.PlanBuilder, dyb, VD) -> list:
        """the dense blocks, last to first: each block's data gradient (a dense block over its stacked-gradient buffer ``dyb(i)``), its
        weight gradient, and the marker of the trunk's upper half"""
        N, H, W, dtc = sp.N, sp.H, sp.W, sp.dtc
        Cc, G, Ccat, R = self.Cc, self.G, self.Ccat, self.R
        VC = VD                              # (the forward's dense-block buffers have the stacked-gradient buffers' layout)
        bw = []
        for i in range(R - 1, -1, -1):
            pre = self._rdb_prefix[i]
            last = self.rrdb and i % 3 == 2
            first = self.rrdb and i % 3 == 0
            s_out = 0.2 if last else 1.0
            ci, di = sp.catb(i), dyb(i)
            blk = []
            for step in range(4):
                kdim = Cc + step * G
                blk.append(ops.conv_args(dtc, VD(di), VD(di, c0=Cc + step * G), b.Wp(("b", i, step)), N, H, W, kdim, G,
                                         mask=VC(ci, c0=Cc + (3 - step) * G), mask_slope=0.2))
            dst = VD(dyb(i - 1)) if i > 0 else A.view(sp.dx0)
            kw = dict(r1=VD(di), r1_scale=s_out)
            if first:
                kw.update(r2=VD(dyb(i + 2)), r2_scale=1.0)
            blk.append(ops.conv_args(dtc, VD(di), dst, b.Wp(("b", i, 4)), N, H, W, Ccat, Cc, **kw))
            chain = ops.dense_chain_or_launches(blk, sp.device) if (Cc, G) == (64, 32) else [ops.Conv(a) for a in blk]
            wg = ops.Wgrad(self._dense_plan(sp, b, self._block_s5(i)), VC(ci), VD(di), dw_off=self._poff(pre + "conv1.weight"), block=i)     # the plan's offsets are relative to the block
            ready = [ops.Ready(self._poff(pre + "conv1.weight"), self._trunk_end())] if self.full and R >= 4 and i == R // 2 else []     # upper half of the trunk is final: second bucket
            # the weight gradient reads what the four growth layers of the data gradient wrote and follows them (or the one launch for all five convs)
            bw.extend(chain[:4] + [wg] + ready + chain[4:])
        return bw

    def _batch_dense_wgrads(self, sp: _Shape, b: ops.PlanBuilder, bw: list, p0: ops.WgradPlan) -> list:
        """``bw`` with the dense blocks' weight gradients batched as the switches say (batch_wgrads / batch_reductions), and the
        workspaces that takes: _BATCH_REDUCE more of the dense-block plan's size (34 MB each at B=32, 128x128)"""
        dense_ws = max((p_.workspace_bytes for p_ in sp.dense_plans.values()), default=0)
        sp.wg_ws4 = [b.buf(dense_ws, dtype=torch.uint8) for _ in range(_BATCH_REDUCE)] if (dense_ws and _BATCH_REDUCE > 1) else None
        if sp.wg_ws4 is None:
            return bw
        if sp.batch_wgrad:
            # a batch of n blocks: plans with 1 / n of one block's pixel splits, so the launch has one block's workgroups
            return batch_wgrads(bw, sp.wg_ws4, lambda wg, n: wg.plan if n == 1 else self._dense_plan(sp, b, self._block_s5(wg.block), max(1, p0.splits // n)))
        return batch_reductions(bw, sp.wg_ws4)

    # -- what a generator with a stage between the trunk and conv2 overrides (engine_trans.py); here: no stage -----------------
    def _stage_pack(self, pb: "ops.PackBuilder", dtc: int) -> None:
        """the stage's packed operands"""

    def _stage_forward(self, sp: _Shape, b: ops.PlanBuilder, fw: list, trunk_out: A.View, train: bool) -> A.View:
        """appends the stage's forward items to ``fw``; returns the view conv2 reads"""
        return trunk_out

    def _conv2_dgrad_target(self, sp: _Shape, trunk_grad: A.View) -> Tuple[A.View, dict]:
        """(where conv2's data gradient goes, its epilogue keywords)"""
        return trunk_grad, {}

    def _stage_backward(self, sp: _Shape, b: ops.PlanBuilder, trunk_grad: A.View) -> list:
        """the stage's backward items, from conv2's data gradient to channels [0, Cc) of ``trunk_grad``, and their bucket marker"""
        return []

    def _trunk_end(self) -> int:
        """offset of the first parameter behind the trunk's"""
        return self._poff("conv2.weight")

    def _finish_backward(self, sp: _Shape, b: ops.PlanBuilder) -> None:
        """last step of _plan_backward, before the workspaces are sized"""

    # -- execution ----------------------------------------------------------------------------
    def trunk_size(self, shape) -> Tuple[int, int, int]:
        """The input shape contract, checked on the host before anything is planned, allocated or launched: the full generator takes
        (N, in_ch / unshuffle^2, H, W) images with H and W multiples of the unshuffle factor, a stand-alone dense block (N, Cc, H, W)
        feature maps.  Returns the (N, H, W) the dense blocks run at."""
        shape = tuple(shape)
        u = self.unshuffle
        want_c = self.in_ch // (u * u) if self.full else self.Cc
        what = self.what
        if len(shape) != 4:
            raise A.SrganfdError(f"{what} expects a 4-D (N, {want_c}, H, W) input, got shape {shape}")
        N, c, H, W = shape
        if c != want_c:
            raise A.SrganfdError(f"{what} expects (N, {want_c}, H, W) inputs, got shape {shape}")
        if H % u or W % u:
            raise A.SrganfdError(f"generator with PixelUnshuffle({u}) expects H and W divisible by {u}: (N, {want_c}, {u}k, {u}m), "
                                 f"got shape {shape}")
        return N, H // u, W // u

    def output_shape(self, shape) -> Tuple[int, int, int, int]:
        """Shape of what forward() returns for an input of ``shape`` (checked as trunk_size() does)."""
        N, H, W = self.trunk_size(shape)
        if not self.full:
            return (N, self.Cc, H, W)
        return (N, self.out_ch, H << self.n_up, W << self.n_up)

    def _check_input(self, x: Tensor) -> Tuple[int, int, int]:
        return self.trunk_size(x.shape)

    def backward(self, sp: _Shape, token: int, dout: Tensor, need_wgrad: bool, need_dx: bool, on_ready=None) -> Tuple[Tensor, Optional[Tensor]]:
        # the weight gradients are always computed: the dense blocks' WgradPartial / WgradReduce do not look at the flag, so a pass with
        # frozen parameters launches what it always has (skipping them would change what is launched: a change of its own)
        return super().backward(sp, token, dout, True, need_dx, on_ready)


# dense blocks whose weight-gradient slabs one srganfd_wgrad_reduce_batch launch reduces (<= 8 = SRGANFD's kRedBatch; 0 / 1: every block's own)
_BATCH_REDUCE = max(0, min(8, int(os.environ.get("SRGANFD_BATCH_REDUCE", "4"))))


def batch_reductions(items: Sequence, slots: Sequence[Tensor]) -> list:
    """The generator's backward list with the dense blocks' weight gradients (ops.Wgrad with a ``block``) as the MFMA launch alone
    (ops.WgradPartial, slabs into the next free workspace of ``slots``) and one ops.WgradReduce per batch: after len(slots) of them,
    before a launch that shares workspace slot 0 (any other weight gradient; a thin launch, which keeps the padded path's order),
    before every gradient bucket is announced, and at the end."""
    out, pending = [], []

    def reduce_pending():
        if pending:
            out.append(ops.WgradReduce(pending))
            pending.clear()
    for it in items:
        if isinstance(it, ops.Wgrad) and it.block is not None:
            pending.append(ops.WgradPartial(it, len(pending), slots[len(pending)]))
            out.append(pending[-1])
            if len(pending) == len(slots):
                reduce_pending()
            continue
        if isinstance(it, (ops.Wgrad, ops.ThinLaunch, ops.Ready)):
            reduce_pending()
        out.append(it)
    reduce_pending()
    return out


# the MFMA launches of those blocks as ONE launch too (batch_wgrads): "0" never, "1" always, "auto" where one block's launch fills the chip
_BATCH_WGRAD = os.environ.get("SRGANFD_BATCH_WGRAD", "auto")


def _written(it) -> set:
    """addresses of the buffers a backward item writes (its output views' base pointers)"""
    if isinstance(it, ops.Conv):
        return {it.args.y.ptr, it.args.y2.ptr} - {None}
    if isinstance(it, ops.DenseChain):
        return ({a.y.ptr for a in it.layers} | {a.y2.ptr for a in it.layers}) - {None}
    if isinstance(it, ops.ThinLaunch):
        return {it.args.big.ptr} if it.op == "thin_in" else set()
    if isinstance(it, ops.Call):                     # auxiliary kernels: every view they take counts as written
        return {a.ptr for a in it.args if isinstance(a, A.View)} - {None}
    return set()


def batch_wgrads(items: Sequence, slots: Sequence[Tensor], plan_for) -> list:
    """batch_reductions with the MFMA launches batched as well: the dense blocks' weight gradients between two of its flush points
    (len(slots) of them; another weight gradient or thin launch; a gradient bucket; the end) become ONE ops.WgradPartialBatch where the
    LAST of them stood, followed by their ops.WgradReduce.  ``plan_for(wg, n)``: the plan block ``wg`` runs with in a batch of n.
    The launch reads every block's stacked gradients later than the block's own launch did: the list is checked -- nothing between
    the place a block's weight gradient had and its batch's launch may write that block's gradient buffer."""
    groups, cur = [], []

    def close():
        if cur:
            groups.append(list(cur))
            cur.clear()
    for idx, it in enumerate(items):
        if isinstance(it, ops.Wgrad) and it.block is not None:
            cur.append(idx)
            if len(cur) == len(slots):
                close()
        elif isinstance(it, (ops.Wgrad, ops.ThinLaunch, ops.Ready)):
            close()
    close()
    last = {g[-1]: g for g in groups}
    member = {idx for g in groups for idx in g}
    out, stood = [], {}                              # stood: index in ``out`` where a block's own weight gradient would have been
    for idx, it in enumerate(items):
        if idx not in member:
            out.append(it)
            continue
        stood[idx] = len(out)
        g = last.get(idx)
        if g is None:
            continue
        parts = [ops.WgradPartial(ops.Wgrad(plan_for(items[j], len(g)), items[j].x, items[j].dy, dw_off=items[j].dw_off, block=items[j].block),
                                  slot, slots[slot]) for slot, j in enumerate(g)]
        for j, p in zip(g, parts):
            for k in range(stood[j], len(out)):
                if p.dy.ptr in _written(out[k]) or p.x.ptr in _written(out[k]):
                    raise A.SrganfdError(f"batched weight gradient: block {items[j].block}'s buffers are overwritten by backward item {k} "
                                         f"({out[k].kind}) before the batch's launch reads them")
        out.append(ops.WgradPartialBatch(parts))
        out.append(ops.WgradReduce(parts))
    return out


class _EngineFn(torch.autograd.Function):
    """An engine's forward(x, *args) under autograd: differentiable in the input and the parameters.  Where forward returns a tuple
    (SelfAttention: the weights), the first element is the result and the rest is handed over beside it, detached.  engine_apply is
    the only caller and asks a generator for a training plan, so a backward through a forward that ran without gradients cannot
    happen (a plan without a backward list has no token, and EngineBase.backward's token check would refuse it)."""

    @staticmethod
    def forward(ctx, x, eng, args, *params):
        out = eng.forward(x, *args)
        ctx.eng, ctx.sp, ctx.token = eng, eng._last, eng.token
        ctx.need_dx, ctx.need_w = ctx.needs_input_grad[0], any(ctx.needs_input_grad[3:])
        if isinstance(out, tuple):
            ctx.mark_non_differentiable(*(t for t in out[1:] if t is not None))
        return out

    @staticmethod
    def backward(ctx, dout, *_):
        g, dx = ctx.eng.backward(ctx.sp, ctx.token, dout, ctx.need_w, ctx.need_dx)
        grads = tuple(ctx.eng.fp.grad_views(g)) if g is not None else (None,) * len(ctx.eng.fp.params)
        unused = getattr(ctx.eng, "unused_params", None)          # registered parameters the forward never reads: None, as autograd gives
        if unused:
            grads = tuple(None if i in unused else t for i, t in enumerate(grads))
        return (dx, None, None) + grads


def _engine(owner: nn.Module, factory):
    eng = _ENGINES.get(owner)
    if eng is None:
        eng = factory()
        # the registry is keyed weakly by the module; the engine must not keep the module alive in turn, or the entry --
        # and every activation buffer of the engine -- would never be released (found at 286 GB by test_fullsize_gpu.py)
        if getattr(eng, "owner", None) is owner:
            eng.owner = weakref.proxy(owner)
        if hasattr(eng, "rdbs"):                      # a stand-alone dense block is its own engine's only block
            eng.rdbs = [weakref.proxy(m) if m is owner else m for m in eng.rdbs]
        _ENGINES[owner] = eng
    return eng


def engine_apply(eng: EngineBase, x: Tensor, *args):
    """A module's forward: through autograd when the input or a parameter wants a gradient.  ``args``: what the engine's forward takes
    after x (a discriminator's ``training``, SelfAttention's ``need_weights``); none for a generator, whose ``train`` is the answer"""
    train = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in eng.fp.params))
    args = args or (train,)
    if not train:
        return eng.forward(x, *args)
    return _EngineFn.apply(x, eng, args, *eng.fp.params)


def trunk_apply(owner: nn.Module, x: Tensor, rdbs: Sequence[nn.Module], rrdb: bool) -> Tensor:
    return engine_apply(_engine(owner, lambda: TrunkEngine(owner, rdbs, rrdb, full=False)), x)


def generator_engine(owner: nn.Module) -> TrunkEngine:
    def make():
        rdbs = []
        for blk in owner.trunk:
            rdbs += [blk.rdb1, blk.rdb2, blk.rdb3]
        from . import model as M
        if isinstance(owner, M.BSRGANtrans):              # (a subclass too: a plain TrunkEngine would silently skip the stage)
            from .engine_trans import TransGeneratorEngine
            return TransGeneratorEngine(owner, rdbs)
        return TrunkEngine(owner, rdbs, rrdb=True, full=True)
    return _engine(owner, make)


def generator_apply(owner: nn.Module, x: Tensor) -> Tensor:
    return engine_apply(generator_engine(owner), x)


def discriminator_apply(owner: nn.Module, x: Tensor) -> Tensor:
    from .engine_d import discriminator_apply as f
    return f(owner, x)


def content_loss_apply(owner: nn.Module, sr: Tensor, gt: Tensor) -> Tensor:
    from .engine_v import content_loss_apply as f
    return f(owner, sr, gt)
