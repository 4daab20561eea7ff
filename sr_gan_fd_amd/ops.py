"""Thin host-side wrappers over the C ABI: weight packing, fused conv, weight gradients.

Host code is plumbing only (device memory, streams); all arithmetic runs in libsrganfd_hip.so.
"""
from __future__ import annotations

import ctypes as C
import os
import struct
from typing import List, Optional, Sequence

import torch

from . import _abi as A
from . import profiling

DT = {torch.bfloat16: A.BF16, torch.float32: A.F32, torch.float16: A.F16}


def esize(dtype_code: int) -> int:
    return 4 if dtype_code == A.F32 else 2


def struct_array_to_device(arr, device) -> torch.Tensor:
    """Upload a ctypes array of PODs; returns the uint8 device tensor that owns the bytes."""
    raw = bytes(memoryview(arr).cast("B"))
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)


class PackTable:
    """A device-resident table of pack jobs (offset based, reusable every step)."""

    def __init__(self, jobs: Sequence[A.PackJob], device):
        self.n = len(jobs)
        arr = (A.PackJob * self.n)(*jobs)
        self.max_elems = max(j.ksize * j.ksize * j.k * j.n for j in jobs)
        self.dev = struct_array_to_device(arr, device)

    def run(self, params: torch.Tensor, packed: torch.Tensor, scalars: Optional[torch.Tensor] = None):
        A.check(A.lib().srganfd_pack_weights(self.dev.data_ptr(), self.n, self.max_elems, params.data_ptr(),
                                             scalars.data_ptr() if scalars is not None else None,
                                             packed.data_ptr(), A.stream_ptr()), "pack_weights")


def pack_job(dst_off: int, dtype: int, ksize: int, k: int, n: int, segs: Sequence[dict]) -> A.PackJob:
    j = A.PackJob()
    j.dst_off, j.dtype, j.ksize, j.k, j.n, j.nseg = dst_off, dtype, ksize, k, n, len(segs)
    # B-fragment order the consuming kernel reads: 16x16x32 fragments for bf16 / f16, 32x32x2 for f32 (the library says which)
    j.layout = A.lib().srganfd_pack_layout(dtype, ksize, n)
    assert 1 <= len(segs) <= 5 and dst_off % 16 == 0
    for i, s in enumerate(segs):
        g = j.seg[i]
        g.src_off = s["src_off"]; g.scale_off = s.get("scale_off", -1)
        g.co_src, g.ci_src = s["co_src"], s["ci_src"]
        g.k_lo, g.k_len = s.get("k_lo", 0), s["k_len"]
        g.co_off, g.ci_off = s.get("co_off", 0), s.get("ci_off", 0)
        g.transposed = s.get("transposed", 0); g.scale = s.get("scale", 1.0)
    return j


def packed_bytes(dtype: int, ksize: int, k: int, n: int) -> int:
    return ksize * ksize * k * n * esize(dtype)


def pad32(c: int) -> int:
    return (c + 31) // 32 * 32


class PackBuilder:
    """Accumulates the pack jobs of one engine and compute dtype: every operand gets the next 256-byte aligned offset of one packed
    buffer under a key of the engine's choice.  ``finish`` returns the record the engines keep per dtype: the device-resident job
    table, the offsets and the (still unwritten) packed buffer."""

    def __init__(self, dtc: int):
        self.dtc, self.jobs, self.offs, self.cur = dtc, [], {}, 0

    def add(self, key, ksize: int, k: int, n: int, segs) -> None:
        self.offs[key] = self.cur
        self.jobs.append(pack_job(self.cur, self.dtc, ksize, k, n, [segs] if isinstance(segs, dict) else segs))
        self.cur += (packed_bytes(self.dtc, ksize, k, n) + 255) // 256 * 256

    def fwd(self, key, src_off: int, co: int, ci: int, ksize: int = 3, **seg) -> None:
        """forward operand of a (co, ci, ksize, ksize) weight at element ``src_off`` of the flat parameters, both sides padded to 32"""
        self.add(key, ksize, pad32(ci), pad32(co), dict(src_off=src_off, co_src=co, ci_src=ci, k_len=pad32(ci), **seg))

    def bwd(self, key, src_off: int, co: int, ci: int, ksize: int = 3, transposed: int = 1, **seg) -> None:
        """data-gradient operand of the same weight (``transposed``: the pack code, 1 = plain transpose with flipped taps)"""
        self.add(key, ksize, pad32(co), pad32(ci), dict(src_off=src_off, co_src=co, ci_src=ci, k_len=pad32(co), transposed=transposed, **seg))

    def classes(self, key: tuple, src_off: int, co: int, ci: int, ksize: int, code: int, **seg) -> None:
        """the four output-parity class operands of a strided conv's data gradient (or of a nearest-x2 forward), back to back under
        ``key + (class,)``: pack codes ``code .. code + 3``, ``ksize`` the classes' tap size"""
        for par in range(4):
            self.bwd(key + (par,), src_off, co, ci, ksize, transposed=code + par, **seg)

    def finish(self, device) -> dict:
        return dict(table=PackTable(self.jobs, device), offs=self.offs, buf=torch.empty(self.cur, dtype=torch.uint8, device=device))


def pack_single(weight: torch.Tensor, dtype: int, transposed: bool = False, scale: float = 1.0) -> torch.Tensor:
    """Pack one (Cout, Cin, k, k) fp32 weight for conv2d (forward) or for its data gradient."""
    co, ci, kh, kw = weight.shape
    assert kh == kw
    k, n = (pad32(co), pad32(ci)) if transposed else (pad32(ci), pad32(co))
    out = torch.empty(packed_bytes(dtype, kh, k, n), dtype=torch.uint8, device=weight.device)
    w = weight.detach().contiguous().float()
    job = pack_job(0, dtype, kh, k, n, [dict(src_off=0, co_src=co, ci_src=ci, k_len=k, transposed=int(transposed), scale=scale)])
    PackTable([job], weight.device).run(w, out)
    return out


def conv_args(dtype: int, x: A.View, y: A.View, w_packed, n: int, h_in: int, w_in: int, cin: int, cout: int, *,
              cout_store: Optional[int] = None, ksize: int = 3, stride: int = 1, pad: int = 1, up: int = 0,
              bias=None, act: int = A.ACT_NONE, slope: float = 0.2, alpha: float = 1.0, post_scale: float = 1.0,
              r1: A.View = A.NULL_VIEW, r1_scale: float = 0.0, r2: A.View = A.NULL_VIEW, r2_scale: float = 0.0,
              mask: A.View = A.NULL_VIEW, mask_slope: float = 0.2, alpha_dev=None, y_f32: bool = False,
              y2: A.View = A.NULL_VIEW) -> A.ConvArgs:
    a = A.ConvArgs()
    a.dtype, a.n, a.h_in, a.w_in, a.up = dtype, n, h_in, w_in, up
    a.ksize, a.stride, a.pad, a.cin, a.cout = ksize, stride, pad, cin, cout
    a.cout_store = cout if cout_store is None else cout_store
    hl, wl = h_in << up, w_in << up
    a.h_out, a.w_out = (hl + 2 * pad - ksize) // stride + 1, (wl + 2 * pad - ksize) // stride + 1
    a.x, a.y, a.r1, a.r2, a.mask, a.y2 = x, y, r1, r2, mask, y2
    a.w_packed = w_packed if isinstance(w_packed, int) else w_packed.data_ptr()
    a.bias = None if bias is None else (bias if isinstance(bias, int) else bias.data_ptr())
    a.alpha_dev = None if alpha_dev is None else (alpha_dev if isinstance(alpha_dev, int) else alpha_dev.data_ptr())
    a.alpha, a.slope, a.post_scale, a.r1_scale, a.r2_scale, a.mask_slope = alpha, slope, post_scale, r1_scale, r2_scale, mask_slope
    a.act, a.y_f32 = act, int(y_f32)
    return a


CLASS4_ENABLED = os.environ.get("SRGANFD_CLASS4", "1") != "0"   # same-box A/B switch: 0 launches the four parity classes separately


def class4_ok(dtype: int, n_out: int, offsets: Sequence[int], pack_bytes: int, ksize: int = 2) -> bool:
    """can the four output-parity classes of a stride-2 data gradient go out as ONE launch (srganfd_conv_args.out_classes = 4)?
    16-bit modes, 2x2- or 1x1-tap classes, the output's channel blocks (64 wide for the 2x2 kernel over a multiple of 64 channels,
    else 32) a power of two, the four packed operands back to back."""
    if n_out % 32:
        return False
    nb = n_out // (64 if ksize == 2 and n_out % 64 == 0 else 32)
    return (CLASS4_ENABLED and dtype != A.F32 and ksize in (1, 2) and nb > 0 and nb & (nb - 1) == 0
            and all(offsets[c] == offsets[0] + c * pack_bytes for c in range(4)))


def parity_class_launches(dtc: int, x: A.View, y: A.View, wptr: int, offs4: Sequence[int], n: int, h: int, w: int, kdim: int, ndim: int,
                          ksize: int, class_pad: int, valid: bool = False, tag: str = "", **epilogue) -> List["Conv"]:
    """A strided conv's data gradient, or a nearest-x2 conv's forward, as its four output-parity classes: stride-1 ``ksize``-tap
    convs over the (h, w) input ``x``, class (py, px) writing the pixels (2i + py, 2j + px) of ``y``.  ``offs4``: byte offsets of the
    four packed operands behind ``wptr``.  ``class_pad`` 1: class (py, px) reads the window one row / column earlier where py / px is
    0 (3x3 and 4x4 pad-1 kernels); 0: every class reads the same window (2x2 stride-2 kernels).  ``valid``: the strided conv had no
    padding (4x4 stride 2 over an even size) -- each class then has one more row and column of outputs, takes the tap pairs of the
    opposite parity and one row / column of zero padding on the low side.  ONE launch when the library takes the four classes
    together (class4_ok), else one per class.  ``tag``: the layer form profiling.conv_label adds to the kernel's name; ``epilogue``:
    conv_args' bias / act / slope / r1 / r2 / mask keywords.  Returns the launches' items."""
    one = not valid and class4_ok(dtc, ndim, offs4, packed_bytes(dtc, ksize, kdim, ndim), ksize)
    ext = 1 if valid else 0
    out = []
    for par in range(1 if one else 4):
        py, px = par >> 1, par & 1
        a = conv_args(dtc, x, y, wptr + offs4[3 - par if valid else par], n, h, w, kdim, ndim, ksize=ksize, stride=1, pad=0, **epilogue)
        a.h_out, a.w_out = h + ext, w + ext
        a.out_sy, a.out_sx, a.out_oy, a.out_ox = 2, 2, py, px
        a.out_h_full, a.out_w_full = 2 * (h + ext), 2 * (w + ext)
        a.pad_y, a.pad_x = (1, 1) if valid else (class_pad * (1 - py), class_pad * (1 - px))
        a.out_classes, a.class_pad_step = (4, class_pad) if one else (0, 0)     # one launch: the classes' workgroups share each input patch through L2
        a._label_tag = tag
        out.append(Conv(a))
    return out


def dgrad_epilogue(r1: Optional[A.View] = None, r2: Optional[A.View] = None, mask: Optional[A.View] = None, mask_slope: float = 0.2) -> dict:
    """conv_args' keywords of a data-gradient epilogue: up to two gradients added at scale 1 and the activation derivative of ``mask``"""
    kw = {}
    if r1 is not None:
        kw.update(r1=r1, r1_scale=1.0)
    if r2 is not None:
        kw.update(r2=r2, r2_scale=1.0)
    if mask is not None:
        kw.update(mask=mask, mask_slope=mask_slope)
    return kw


def conv2d(args: A.ConvArgs, rec=None, what: str = "conv2d", L=None, st=None) -> None:
    """Issue one conv launch on the current stream; ``rec`` (profiling.REC) brackets it with its label and algorithmic work.  A loop
    over many launches passes the library handle and the stream it already holds."""
    if L is None:
        L, st = A.lib(), A.stream_ptr()
    if rec is None:
        rc = L.srganfd_conv2d(C.byref(args), st)
        if rc:
            A.check(rc, what)
    else:
        rec.bracket(profiling.conv_label(args), profiling.conv_work(args), lambda: A.check(L.srganfd_conv2d(C.byref(args), st), what))


# ---- launch items: what the engines' per-shape launch lists (sp.fw / sp.bw) hold.  Every item has ``launch(run)`` and ``run_items`` is
# the one loop over a list; ``kind`` names the class for tests and debugging, nothing dispatches on it.  Here: Conv, Call, Wgrad,
# WgradPartial / WgradPartialBatch / WgradReduce (the generator's dense blocks: batched MFMA launch, batched slab reduction), Ready (the generator's gradient buckets), PerCall (a
# layer that writes the pass's own output) and, further down, DenseChain, ThinLaunch, Attention, PixelGate, SeqAttention, AddLayerNorm and DropoutApply; the engines define the items only they launch
# beside themselves (BatchNorm, the spectral-norm gradient, the loss taps).  An item holds structs and addresses, never a closure:
# what the addresses point to is kept alive by the plan's buffers.
class Run:
    """What one pass over a launch list needs besides the items: the library handle, the stream and profiling.REC; ``what``: the name
    A.check reports for the list's convs; the ``training`` / ``need_wgrad`` flags of the pass; the addresses that exist per call only
    -- ``grad`` (the flat gradient), ``scratch`` (where a spectral-normalised layer's weight gradient goes first) and ``out`` (the
    logits, the loss vector); ``ws``: the workspace the list's weight-gradient launches share; ``on_ready(lo, hi)``: told when
    elements [lo, hi) of the flat gradient are final."""
    __slots__ = ("L", "st", "rec", "what", "training", "need_wgrad", "grad", "scratch", "out", "ws", "on_ready")

    def __init__(self, what: str, training: bool = False, need_wgrad: bool = True, grad: int = 0, scratch: int = 0, out: int = 0,
                 ws: Optional[torch.Tensor] = None, on_ready=None):
        self.L, self.st, self.rec = A.lib(), A.stream_ptr(), profiling.REC
        self.what, self.training, self.need_wgrad = what, training, need_wgrad
        self.grad, self.scratch, self.out, self.ws, self.on_ready = grad, scratch, out, ws, on_ready


def run_items(items: Sequence, run: Run) -> None:
    for item in items:
        item.launch(run)


class Conv:
    """one fused-conv launch"""
    __slots__ = ("args",)
    kind = "conv"

    def __init__(self, args: A.ConvArgs):
        self.args = args

    def launch(self, run: Run) -> None:
        conv2d(self.args, run.rec, run.what, run.L, run.st)

    def set_output(self, ptr: int) -> None:
        self.args.y.ptr = ptr


class PerCall:
    """a Conv, thin_out ThinLaunch or Attention whose output is the pass's own (``run.out``: allocated per call), put into the struct at
    launch; skipped by a pass that did not ask for that output (``run.out`` 0)"""
    __slots__ = ("item",)
    kind = "per_call"

    def __init__(self, item):
        self.item = item

    def launch(self, run: Run) -> None:
        if run.out:
            self.item.set_output(run.out)
            self.item.launch(run)


class Call:
    """an auxiliary kernel: the C entry point's name, its arguments without the trailing stream, and what A.check reports (never bracketed)"""
    __slots__ = ("name", "args", "what")
    kind = "call"

    def __init__(self, name: str, args: tuple, what: str):
        self.name, self.args, self.what = name, args, what

    def launch(self, run: Run) -> None:
        A.check(getattr(run.L, self.name)(*self.args, run.st), self.what)


class Ready:
    """marker of the generator's backward list: every launch that writes elements [lo, hi) of the flat gradient has been enqueued"""
    __slots__ = ("lo", "hi")
    kind = "ready"

    def __init__(self, lo: int, hi: int):
        self.lo, self.hi = lo, hi

    def launch(self, run: Run) -> None:
        if run.on_ready is not None:
            run.on_ready(self.lo, self.hi)


class Wgrad:
    """one weight-gradient launch of ``plan`` over the views x / dy, skipped by a pass with frozen parameters.  ``dw_off``: elements
    added to the flat gradient's base (the generator's dense-block plans hold offsets relative to their block); ``sn``: the
    spectral-norm slot of a discriminator layer, whose gradient goes to the scratch buffer first, or None; ``block``: the generator's
    dense-block index (engine.batch_reductions turns these into WgradPartial + WgradReduce), or None"""
    __slots__ = ("plan", "x", "dy", "dw_off", "sn", "block")
    kind = "wgrad"

    def __init__(self, plan: "WgradPlan", x: A.View, dy: A.View, dw_off: int = 0, sn: Optional[int] = None, block: Optional[int] = None):
        self.plan, self.x, self.dy, self.dw_off, self.sn, self.block = plan, x, dy, dw_off, sn, block

    def launch(self, run: Run) -> None:
        if run.need_wgrad:
            conv2d_wgrad(self.plan, self.x, self.dy, (run.grad if self.sn is None else run.scratch) + 4 * self.dw_off, run.ws, run.rec, run.L, run.st)


class _Bracketed:
    """base of the items profiling.REC brackets under their ``label`` and algorithmic ``work``; ``_issue(run)`` makes the call"""

    def launch(self, run: Run) -> None:
        if run.rec is None:
            self._issue(run)
        else:
            run.rec.bracket(self.label, self.work, lambda: self._issue(run))


class WgradPartial(_Bracketed):
    """a dense block's weight-gradient MFMA launch alone: the slabs stay in ``ws``, workspace ``slot`` of the batch a WgradReduce reduces"""
    kind = "wgrad_partial"

    def __init__(self, wg: Wgrad, slot: int, ws: torch.Tensor):
        self.plan, self.x, self.dy, self.dw_off, self.block, self.slot, self.ws = wg.plan, wg.x, wg.dy, wg.dw_off, wg.block, slot, ws
        self.label, self.work = wg.plan.label, (wg.plan.flops, wg.plan.nbytes)

    def _issue(self, run: Run) -> None:
        plan, ws = self.plan, self.ws
        A.check(run.L.srganfd_conv2d_wgrad_partial(plan.host, plan.dev.data_ptr(), self.x, self.dy, ws.data_ptr(), ws.numel(), run.st), "conv2d_wgrad_partial")


class WgradPartialBatch(_Bracketed):
    """the weight-gradient MFMA launches of up to SRGANFD's kRedBatch dense blocks as ONE launch (srganfd_conv2d_wgrad_partial_batch):
    ``partials`` are the blocks' WgradPartial items, which are not in the list themselves -- their plans share geometry, pixel splits
    and channel groups (engine.batch_wgrads builds them with 1 / n of one launch's splits), each keeps its own workspace, and a
    WgradReduce over the same partials follows.  Bracketed under the plan's label with the jobs' summed work."""
    kind = "wgrad_partial_batch"

    def __init__(self, partials: Sequence[WgradPartial]):
        self.partials, self.n = list(partials), len(partials)
        self.jobs = (A.WgradPartialJob * self.n)()
        for j, p in zip(self.jobs, self.partials):
            j.plan_host, j.plan_dev, j.x, j.dy = C.addressof(p.plan.host), p.plan.dev.data_ptr(), p.x, p.dy
            j.workspace, j.workspace_bytes = p.ws.data_ptr(), p.ws.numel()
        self.label = self.partials[0].label
        self.work = (sum(p.work[0] for p in self.partials), sum(p.work[1] for p in self.partials))

    def _issue(self, run: Run) -> None:
        A.check(run.L.srganfd_conv2d_wgrad_partial_batch(self.jobs, self.n, run.st), "conv2d_wgrad_partial_batch")


class WgradReduce(_Bracketed):
    """the slab reduction of up to SRGANFD's kRedBatch WgradPartial launches as ONE launch (the reduction is latency-bound at ~20 us
    whatever it reduces).  The job array is built with the plan; a launch fills in where the pass's flat gradient is."""
    kind, label = "wgrad_reduce", "wgrad_reduce_batch"

    def __init__(self, partials: Sequence[WgradPartial]):
        self.partials, self.n = list(partials), len(partials)
        self.jobs = (A.WgradReduceJob * self.n)()
        for j, p in zip(self.jobs, self.partials):
            j.plan_host, j.plan_dev, j.scalars, j.workspace = C.addressof(p.plan.host), p.plan.dev.data_ptr(), None, p.ws.data_ptr()
        self.work = (0.0, float(sum(p.ws.numel() for p in self.partials)))

    def _issue(self, run: Run) -> None:
        for j, p in zip(self.jobs, self.partials):
            j.grads = run.grad + 4 * p.dw_off
        A.check(run.L.srganfd_wgrad_reduce_batch(self.jobs, self.n, run.st), "wgrad_reduce_batch")


# ---- LDS-resident dense-block launch (csrc/dense_chain.hip): the five convs of a dense block, or of its data-gradient pass, as one launch ----
DENSE_CHAIN = os.environ.get("SRGANFD_DENSE_CHAIN", "auto")     # "0": never, "1": whenever the arguments qualify, "auto": small launches only (see dense_chain_wanted)
_DC_WS = {}


def dense_chain_workspace(device) -> torch.Tensor:
    """hand-off flags + header (give-up count, epoch, finished-workgroup count) of the dense-chain launches of one device, zeroed once
    here.  The flags are epoch-valued: the last workgroup of a launch advances the epoch, so nothing is zeroed per launch, a captured
    graph replays correctly, and -- the launches running in stream order -- every chain of a device can share it"""
    ws = _DC_WS.get(str(device))
    if ws is None:
        ws = _DC_WS[str(device)] = torch.zeros(int(A.lib().srganfd_dense_chain_workspace_bytes()), dtype=torch.uint8, device=device)
    return ws


def dense_chain_giveups(device):
    """hand-off waits that gave up since the device's workspace was allocated (None: no dense-chain launch was ever planned there);
    synchronises -- for the end of a run, not for the step"""
    ws = _DC_WS.get(str(device))
    return None if ws is None else int(ws[:4].view(torch.int32).item())


def dense_chain_wanted(n: int, h: int, w: int, cus: int = 256) -> bool:
    """the launch needs every 16 x 16 tile of a pass resident at once (one workgroup per CU, cus // tiles images per pass) and keeps
    one flag per growth layer and tile of the call.  "auto" takes it where it measured faster than the five launches
    (profiles/r05_dense_chain_v2_bench.txt): batches that fit ONE pass -- 1.5x (forward) / 1.35x (data gradient) at the reference's
    crop sizes; a second pass costs a whole pass whatever it holds (batch 16 at 72 x 72: 400 tiles, 0.96x / 0.83x) and at batch 32,
    128 x 128 (eight passes) the per-layer launches are 1.2x faster"""
    if DENSE_CHAIN == "0":
        return False
    per = -(-h // 16) * -(-w // 16)
    if per > cus or n * per > 16384:
        return False
    return DENSE_CHAIN == "1" or n * per <= cus


class DenseChain(_Bracketed):
    """n conv launches (A.ConvArgs, the arguments srganfd_conv2d would get) run by srganfd_dense_chain; ``ok`` False when the library
    refuses them (then the caller keeps the separate launches)."""
    kind = "chain"

    def __init__(self, layers: Sequence[A.ConvArgs], device):
        self.n = len(layers)
        self.arr = (A.ConvArgs * self.n)()
        for i, a in enumerate(layers):
            C.memmove(C.byref(self.arr, i * C.sizeof(A.ConvArgs)), C.byref(a), C.sizeof(A.ConvArgs))
        self.layers = list(layers)           # keeps the structs (and the label cache on them) alive
        self.ok = A.lib().srganfd_dense_chain_check(self.arr, self.n) == 0
        self.ws = dense_chain_workspace(device) if self.ok else None
        self.flops = sum(2.0 * a.n * a.h_out * a.w_out * 9 * a.cin * a.cout for a in layers)
        # algorithmic bytes of the launch: the block input read once, every layer's output written once, the epilogue operands read once
        es, px = 2, layers[0].n * layers[0].h_out * layers[0].w_out
        self.bytes = float(px * es * (layers[0].cin + sum(a.cout * (1 + bool(a.r1.ptr) + bool(a.r2.ptr) + bool(a.mask.ptr)) for a in layers)))
        self.label = "dense_chain_kernel<%s,%d layers%s>" % (A.DT_NAME[layers[0].dtype], self.n, ",mask" if layers[0].mask.ptr else "")
        self.work = (self.flops, self.bytes)

    def run(self, L=None, st=None) -> None:
        if L is None:
            L, st = A.lib(), A.stream_ptr()
        A.check(L.srganfd_dense_chain(self.arr, self.n, self.ws.data_ptr(), self.ws.numel(), st), "dense_chain")

    def _issue(self, run: Run) -> None:
        self.run(run.L, run.st)

    def errors(self) -> int:
        """hand-off waits that gave up since the workspace was allocated (synchronises; tests)"""
        return int(self.ws[:4].view(torch.int32).item())


def dense_chain_or_launches(layers: Sequence[A.ConvArgs], device) -> list:
    """a dense block's items: [DenseChain] when the batch is in the chain's regime and the library accepts the launches, else a Conv each"""
    a = layers[0]
    if a.dtype in (A.F16, A.BF16) and dense_chain_wanted(a.n, a.h_in, a.w_in):
        ch = DenseChain(layers, device)
        if ch.ok:
            return [ch]
    return [Conv(a) for a in layers]


# ---- thin-side convolutions (csrc/conv_thin.hip): 1..4 channels against 64, 3x3 stride 1 pad 1, 16-bit dtypes ----
THIN_ENABLED = os.environ.get("SRGANFD_THIN", "1") != "0"      # same-box A/B switch: 0 keeps these layers on the 32-channel-padded kernels


def thin_ok(dtype: int, big_channels: int, thin_channels: int, ksize: int = 3) -> bool:
    """does this layer run on the thin kernels?  (16-bit modes, 64 channels against 1..4, 3x3: everything else -- and the exact-fp32
    parity mode -- stays on srganfd_conv2d with the thin side padded to 32 channels)"""
    return THIN_ENABLED and dtype != A.F32 and big_channels == 64 and 1 <= thin_channels <= 4 and ksize == 3


def _ptr(t):
    return None if t is None else (t if isinstance(t, int) else t.data_ptr())


def thin_args(dtype: int, n: int, h: int, w: int, cs: int, weight, big: A.View, *, w_big_is_cout: bool, flip: bool = False, bias=None,
              act: int = A.ACT_NONE, slope: float = 0.2, mask: A.View = A.NULL_VIEW, mask_slope: float = 0.2, thin=None, thin_out=None,
              thin_out_pitch: int = 4) -> A.ThinArgs:
    """weight: the layer's raw fp32 parameter (Cout, Cin, 3, 3) -- tensor or device address; thin: NHWC4 16-bit tensor / address"""
    a = A.ThinArgs()
    a.dtype, a.n, a.h, a.w, a.cs = dtype, n, h, w, cs
    a.w_big_is_cout, a.flip, a.act, a.slope, a.mask_slope = int(w_big_is_cout), int(flip), act, slope, mask_slope
    a.weight, a.bias, a.big, a.mask = _ptr(weight), _ptr(bias), big, mask
    a.thin, a.thin_out, a.thin_out_pitch = _ptr(thin), _ptr(thin_out), thin_out_pitch
    return a


def thin_work(a: A.ThinArgs, kind: str):
    """(algorithmic FLOP, algorithmic bytes) of one thin launch: 2 * pixels * 9 * 64 * cs; 64-channel tensor (+ mask) once, thin tensor once"""
    px = float(a.n) * a.h * a.w
    nbytes = px * (128.0 + (128.0 if a.mask.ptr else 0.0) + (4.0 * a.thin_out_pitch if kind == "thin_out" else 8.0))
    return 2.0 * px * 9 * 64 * a.cs, nbytes


def thin_in(a: A.ThinArgs) -> None:
    A.check(A.lib().srganfd_conv2d_thin_in(C.byref(a), A.stream_ptr()), "conv2d_thin_in")


def thin_out(a: A.ThinArgs) -> None:
    A.check(A.lib().srganfd_conv2d_thin_out(C.byref(a), A.stream_ptr()), "conv2d_thin_out")


def thin_wgrad_workspace_bytes() -> int:
    return int(A.lib().srganfd_conv2d_thin_wgrad_workspace())


def thin_wgrad(a: A.ThinArgs, dw, db, workspace: torch.Tensor) -> None:
    A.check(A.lib().srganfd_conv2d_thin_wgrad(C.byref(a), _ptr(dw), _ptr(db), workspace.data_ptr(), workspace.numel() * workspace.element_size(),
                                              A.stream_ptr()), "conv2d_thin_wgrad")


THIN_OPS = ("thin_in", "thin_out", "thin_wgrad")


def thin_describe(a: A.ThinArgs, op) -> str:
    """label of the kernel instantiation srganfd_conv2d_<op> launches for these arguments (op: 0 / 1 / 2 or a name of THIN_OPS); nothing runs"""
    buf = C.create_string_buffer(96)
    A.check(A.lib().srganfd_conv2d_thin_describe(C.byref(a), op if isinstance(op, int) else THIN_OPS.index(op), buf, 96), "conv2d_thin_describe")
    return buf.value.decode()


def resample_describe(dtype: int, n: int, h: int, w: int, c: int, a: A.View, b: A.View, op=None, *, act: A.View = A.NULL_VIEW,
                      b2: A.View = A.NULL_VIEW) -> str:
    """label, "<kernel>/<dtype>", of the kernel instantiation srganfd_resample(op, a, b, ...) launches for these arguments -- or, with
    ``op`` None, srganfd_resample_bwd_lrelu(dy=a, dx_raw=b, act, dx_masked=b2, ...); nothing runs"""
    buf = C.create_string_buffer(96)
    entry, op = (1, 2) if op is None else (0, op)
    A.check(A.lib().srganfd_resample_describe(entry, op, a, b, act, b2, dtype, n, h, w, c, buf, 96), "resample_describe")
    return buf.value.decode()


class ThinLaunch(_Bracketed):
    """One thin-side launch in an engine's launch list.  op: "thin_in" / "thin_out" / "thin_wgrad" (the latter writes the weight and
    bias gradient at element offsets ``dw_off`` / ``db_off`` of the pass's flat gradient, and is skipped by a pass with frozen parameters)."""
    kind = "thin"

    def __init__(self, op: str, args: A.ThinArgs, dw_off: int = -1, db_off: int = -1, ws: Optional[torch.Tensor] = None):
        self.op, self.args, self.dw_off, self.db_off, self.ws = op, args, dw_off, db_off, ws
        self.is_wgrad = op == "thin_wgrad"
        self.label = "%s_kernel<%s%s>" % (op, A.DT_NAME[args.dtype], ",mask" if args.mask.ptr else "")
        self.work = thin_work(args, op)

    def set_output(self, ptr: int) -> None:
        self.args.thin_out = ptr

    def launch(self, run: Run) -> None:
        if run.need_wgrad or not self.is_wgrad:
            _Bracketed.launch(self, run)

    def _issue(self, run: Run) -> None:
        a, L, st, grad_ptr = self.args, run.L, run.st, run.grad
        if self.op == "thin_in":
            rc = L.srganfd_conv2d_thin_in(C.byref(a), st)
        elif self.op == "thin_out":
            rc = L.srganfd_conv2d_thin_out(C.byref(a), st)
        else:
            rc = L.srganfd_conv2d_thin_wgrad(C.byref(a), grad_ptr + 4 * self.dw_off, (grad_ptr + 4 * self.db_off) if self.db_off >= 0 else None,
                                             self.ws.data_ptr(), self.ws.numel() * self.ws.element_size(), st)
        if rc:
            A.check(rc, self.op)


# ---- image-side layers: a 3x3 conv between an image-like tensor (``cs`` = 1..4 real channels) and ``big_ch`` feature channels.  In the
# 16-bit modes with 64 feature channels (thin_ok) the image side is NHWC with a 4-channel pitch and the thin kernels read the layer's
# raw fp32 ``weight`` (an address in the flat parameters); otherwise it is padded to 32 channels for conv2d and the packed operand.
# ``w_big_is_cout``: the weight's output channels are the feature side (a network's first layer; False: its last).  Each returns one
# launch item: a ThinLaunch, or a Conv / Wgrad.
def image_to_features(dtc: int, thin: bool, image: torch.Tensor, big: A.View, weight: int, w_packed: int, n: int, h: int, w: int, cs: int,
                      big_ch: int, w_big_is_cout: bool, flip: bool = False, **epilogue):
    """a first layer's forward, or (flip) a last layer's data gradient; epilogue: bias / act / slope / mask / mask_slope"""
    if thin:
        return ThinLaunch("thin_in", thin_args(dtc, n, h, w, cs, weight, big, w_big_is_cout=w_big_is_cout, flip=flip, thin=image, **epilogue))
    return Conv(conv_args(dtc, A.view(image), big, w_packed, n, h, w, image.shape[-1], big_ch, **epilogue))


def features_to_image(dtc: int, thin: bool, big: A.View, out, out_pitch: int, weight: int, w_packed: int, n: int, h: int, w: int, cs: int,
                      big_ch: int, w_big_is_cout: bool, flip: bool = False, bias=None):
    """a last layer's forward, or (flip) a first layer's data gradient, written as fp32 at ``out`` (tensor or address) with a pitch of
    ``out_pitch`` channels"""
    if thin:
        return ThinLaunch("thin_out", thin_args(dtc, n, h, w, cs, weight, big, w_big_is_cout=w_big_is_cout, flip=flip, bias=bias,
                                                thin_out=out, thin_out_pitch=out_pitch))
    return Conv(conv_args(dtc, big, A.View(_ptr(out), out_pitch, 0), w_packed, n, h, w, big_ch, 32, cout_store=cs, bias=bias, y_f32=True))


def image_wgrad(dtc: int, thin: bool, wplans: "WgradPlans", image: torch.Tensor, big: torch.Tensor, weight: int, dw_off: int, db_off: int,
                thin_ws: Optional[torch.Tensor], n: int, h: int, w: int, cs: int, big_ch: int, w_big_is_cout: bool):
    """weight and bias gradient of either layer, at elements dw_off / db_off of the flat gradient (held by the plan: the item adds nothing)"""
    if thin:
        return ThinLaunch("thin_wgrad", thin_args(dtc, n, h, w, cs, weight, A.view(big), w_big_is_cout=w_big_is_cout, thin=image),
                          dw_off=dw_off, db_off=db_off, ws=thin_ws)
    if w_big_is_cout:
        return Wgrad(wplans.conv(h, w, image.shape[-1], big_ch, dw_off, db_off, cin_real=cs), A.view(image), A.view(big), dw_off=0, sn=None)
    return Wgrad(wplans.conv(h, w, big_ch, 32, dw_off, db_off, cout_real=cs), A.view(big), A.view(image), dw_off=0, sn=None)


class WgradPlan:
    """Host+device plan of one weight-gradient launch (several convs sharing x and dy)."""

    def __init__(self, device, dtype: int, n: int, h_in: int, w_in: int, x_channels: int, dy_channels: int,
                 convs: Sequence[dict], ksize: int = 3, stride: int = 1, pad: int = 1, up: int = 0, splits: int = 0):
        hl, wl = h_in << up, w_in << up
        s = A.WgradShape(dtype, n, h_in, w_in, up, ksize, stride, pad, (hl + 2 * pad - ksize) // stride + 1,
                         (wl + 2 * pad - ksize) // stride + 1, x_channels, dy_channels, len(convs), splits)
        carr = (A.WgradConv * len(convs))()
        for i, c in enumerate(convs):
            w = carr[i]
            w.ci_lo, w.cin, w.co_lo, w.cout = c.get("ci_lo", 0), c["cin"], c.get("co_lo", 0), c["cout"]
            w.dw_off, w.db_off = c["dw_off"], c.get("db_off", -1)
            w.co_dst, w.ci_dst = c["co_dst"], c["ci_dst"]
            w.alpha, w.beta, w.alpha_off = c.get("alpha", 1.0), c.get("beta", 0.0), c.get("alpha_off", -1)
        ho, wo = s.h_out, s.w_out
        self.flops = sum(2.0 * n * ho * wo * ksize * ksize * c["co_dst"] * c["ci_dst"] for c in convs)
        es = 4 if dtype == A.F32 else 2
        # algorithmic bytes: x and dy read once, fp32 gradients written once
        self.nbytes = float(n * h_in * w_in * x_channels * es + n * ho * wo * dy_channels * es
                            + sum(4.0 * ksize * ksize * c["co_dst"] * c["ci_dst"] for c in convs))
        self.label = f"wgrad_kernel<{A.DT_NAME[dtype]},KS={ksize},S={stride}>+reduce"
        L = A.lib()
        nbytes = L.srganfd_wgrad_plan_bytes(C.byref(s), carr)
        if nbytes == 0:
            raise A.SrganfdError("wgrad plan: " + L.srganfd_last_error().decode())
        self.host = C.create_string_buffer(nbytes)
        ws = C.c_size_t(0)
        A.check(L.srganfd_wgrad_plan_build(C.byref(s), carr, self.host, nbytes, C.byref(ws)), "wgrad_plan_build")
        self.workspace_bytes = ws.value
        self.dev = torch.frombuffer(bytearray(self.host.raw), dtype=torch.uint8).to(device)
        # what the library chose: the plan starts with csrc/wgrad.hip's WgHeader, 32-bit fields -- [11] channel groups (workgroups per
        # pixel split), [13] pixel splits, [17] pixel tiles
        hdr = struct.unpack_from("<18i", self.host.raw)
        self.ngroups, self.splits, self.ntiles = hdr[11], hdr[13], hdr[17]

    def run(self, x: A.View, dy: A.View, grads: torch.Tensor, workspace: torch.Tensor,
            scalars: Optional[torch.Tensor] = None) -> None:
        assert workspace.numel() * workspace.element_size() >= self.workspace_bytes
        A.check(A.lib().srganfd_conv2d_wgrad(self.host, self.dev.data_ptr(), x, dy, grads.data_ptr(),
                                             scalars.data_ptr() if scalars is not None else None,
                                             workspace.data_ptr(), workspace.numel() * workspace.element_size(),
                                             A.stream_ptr()), "conv2d_wgrad")


def conv2d_wgrad(plan: WgradPlan, x: A.View, dy: A.View, grad_ptr: int, workspace: torch.Tensor, rec=None, L=None, st=None) -> None:
    """Issue one weight-gradient launch (MFMA kernel + slab reduction) writing at ``grad_ptr``; ``rec`` brackets it as conv2d's does."""
    if L is None:
        L, st = A.lib(), A.stream_ptr()
    run = lambda: A.check(L.srganfd_conv2d_wgrad(plan.host, plan.dev.data_ptr(), x, dy, grad_ptr, None, workspace.data_ptr(), workspace.numel(), st),
                          "conv2d_wgrad")
    if rec is None:
        run()
    else:
        rec.bracket(plan.label, (plan.flops, plan.nbytes), run)


def device_cus(device) -> int:
    """compute units of ``device``, what the library sizes a weight-gradient launch's pixel splits by (256 in dry runs, as in the library)"""
    if A.DRY_RUN or torch.device(device).type != "cuda":
        return 256
    return int(torch.cuda.get_device_properties(device).multi_processor_count)


class WgradPlans:
    """Builds the weight-gradient plans of one launch list and keeps the largest workspace any of them needs (they run one after the
    other and share it)."""

    def __init__(self, device, dtc: int, n: int):
        self.device, self.dtc, self.n, self.ws_bytes = device, dtc, n, 0

    def plan(self, h: int, w: int, x_channels: int, dy_channels: int, convs: Sequence[dict], **kw) -> WgradPlan:
        p = WgradPlan(self.device, self.dtc, self.n, h, w, x_channels, dy_channels, convs, **kw)
        self.ws_bytes = max(self.ws_bytes, p.workspace_bytes)
        return p

    def conv(self, h: int, w: int, cin: int, cout: int, dw_off: int, db_off: int = -1, cin_real: Optional[int] = None,
             cout_real: Optional[int] = None, **kw) -> WgradPlan:
        """plan of ONE conv whose x / dy carry cin / cout (padded) channels; the gradient of the real (cout_real, cin_real) weight goes
        to element ``dw_off`` of the flat gradient, the bias gradient to ``db_off``"""
        return self.plan(h, w, cin, cout, [dict(cin=cin, cout=cout, dw_off=dw_off, db_off=db_off, co_dst=cout_real or cout, ci_dst=cin_real or cin)], **kw)

    def workspace(self) -> torch.Tensor:
        return torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.device)


def _view(t) -> A.View:
    return t if isinstance(t, A.View) else A.view(t)


class PlanBuilder:
    """What the engines' planners share, made once per plan (EngineBase._plan) from the engine, the plan ``sp`` -- its N, dt, dtc and
    device -- and the packed record ``pk``: the plan's buffers, the addresses of parameters and packed operands, and the launch items
    the planners put into sp.fw / sp.bw.  Where an item takes ``x`` / ``y`` / ``dy`` / ``mask`` ..., a tensor stands for the view of
    all its channels.  ``n``: the batch of the conv and weight-gradient launches where it is not the plan's N (the transformer layers
    run their T tokens as one (S, Nq) image).  ``wplans``: the plan's weight-gradient plans."""

    def __init__(self, eng, sp, pk: dict, n: Optional[int] = None):
        self.N, self.dt, self.dtc, self.device, self.pk = sp.N if n is None else n, sp.dt, sp.dtc, sp.device, pk
        self.poff = eng._poff                                  # a parameter's element offset in the flat parameters and the flat gradient
        self.fptr, self.wptr, self.offs = eng.fp.flat.data_ptr(), pk["buf"].data_ptr(), pk["offs"]
        self.wplans = WgradPlans(self.device, self.dtc, self.N)

    # ---- buffers ----
    def buf(self, *shape, dtype=None) -> torch.Tensor:
        return torch.empty(*shape, dtype=self.dt if dtype is None else dtype, device=self.device)

    def act(self, h: int, w: int, c: int, dtype=None) -> torch.Tensor:
        """an (N, h, w, c) activation or gradient, in the compute dtype unless ``dtype`` says otherwise"""
        return self.buf(self.N, h, w, c, dtype=dtype)

    def thin_ws(self, *thin: bool) -> Optional[torch.Tensor]:
        """the thin weight-gradient workspace, if any of the plan's image-side layers is thin"""
        return torch.empty(thin_wgrad_workspace_bytes(), dtype=torch.uint8, device=self.device) if any(thin) else None

    # ---- addresses ----
    def P(self, name: str) -> int:
        """address of a parameter in the flat buffer"""
        return self.fptr + 4 * self.poff(name)

    def Wp(self, key) -> int:
        """address of a packed operand"""
        return self.wptr + self.offs[key]

    # ---- items ----
    def conv(self, x, y, key, h: int, w: int, cin: int, cout: int, **kw) -> "Conv":
        """one conv launch with the packed operand ``key`` over the (N, h, w, cin) input; ``kw``: conv_args' keywords"""
        return Conv(conv_args(self.dtc, _view(x), _view(y), self.Wp(key), self.N, h, w, cin, cout, **kw))

    def dgrad(self, dy, dx, key, h: int, w: int, cout: int, cin: int, r1=None, r2=None, mask=None, mask_slope: float = 0.2, **kw) -> "Conv":
        """a stride-1 conv's data gradient: reads dy (cout channels), writes dx (cin channels); ``r1`` / ``r2``: gradients added at
        scale 1, ``mask``: the activation whose derivative multiplies the sum (dgrad_epilogue)"""
        ep = dgrad_epilogue(*(None if t is None else _view(t) for t in (r1, r2, mask)), mask_slope)
        return self.conv(dy, dx, key, h, w, cout, cin, **ep, **kw)

    def strided_dgrad(self, dy, dx, key: tuple, hd: int, wd: int, kdim: int, ndim: int, ksize: int, class_pad: int, r1=None, r2=None, mask=None,
                      valid: bool = False) -> List["Conv"]:
        """a stride-2 conv's data gradient as its four output-parity classes (parity_class_launches; the operands under ``key + (class,)``)
        over the (hd, wd) gradient dy, with dgrad's epilogue"""
        ep = dgrad_epilogue(*(None if t is None else _view(t) for t in (r1, r2, mask)))
        return parity_class_launches(self.dtc, _view(dy), _view(dx), self.wptr, [self.offs[key + (c,)] for c in range(4)], self.N, hd, wd, kdim, ndim,
                                     ksize, class_pad, valid=valid, **ep)

    def wgrad(self, x, dy, h: int, w: int, cin: int, cout: int, weight: str, bias: Optional[str] = None, sn: Optional[int] = None,
              cin_real: Optional[int] = None, cout_real: Optional[int] = None, **kw) -> "Wgrad":
        """weight gradient of one conv over the (N, h, w, cin) input x and the gradient dy (cout channels), written at parameter
        ``weight`` (and ``bias``) of the flat gradient; ``sn``: the layer's spectral-norm slot; ``kw``: ksize / stride / pad / up"""
        plan = self.wplans.conv(h, w, cin, cout, self.poff(weight), -1 if bias is None else self.poff(bias), cin_real, cout_real, **kw)
        return Wgrad(plan, _view(x), _view(dy), sn=sn)

    def resample(self, op: int, a, b, h: int, w: int, c: int, dtype: Optional[int] = None, n: Optional[int] = None, what: str = "resample") -> "Call":
        return Call("srganfd_resample", (op, _view(a), _view(b), self.dtc if dtype is None else dtype, self.N if n is None else n, h, w, c), what)

    def lrelu_bwd(self, dy, act, out, npix: int, c: int, slope: float = 0.2) -> "Call":
        return Call("srganfd_lrelu_bwd", (_view(dy), _view(act), A.NULL_VIEW, _view(out), self.dtc, npix, c, slope), "lrelu_bwd")

    def resample_bwd_lrelu(self, dy, raw, act, masked, h: int, w: int, c: int, slope: float = 0.2) -> "Call":
        """bilinear-x2 backward and LeakyReLU' of the upsampled layer in one pass: the raw gradient (a skip connection's share) and the masked one"""
        return Call("srganfd_resample_bwd_lrelu", (_view(dy), _view(raw), _view(act), _view(masked), self.dtc, self.N, h, w, c, slope), "resample_bwd_lrelu")

    # the image-side layers (image_to_features, features_to_image, image_wgrad) of the layer ``name``: ``cs`` real image channels
    # against ``big_ch`` features at (h, w); ``first``: the network's first layer (its weight's output channels are the features);
    # ``flip``: the other layer's data gradient, which takes no bias; ``key``: the packed operand where it is not (direction, name)
    def image_to_features(self, thin: bool, image, big, name: str, h: int, w: int, cs: int, big_ch: int, first: bool, flip: bool = False, key=None,
                          **epilogue):
        bias = {} if flip else dict(bias=self.P(name + ".bias"))
        return image_to_features(self.dtc, thin, image, _view(big), self.P(name + ".weight"), self.Wp(key or ("b" if flip else "f", name)), self.N, h, w,
                                 cs, big_ch, first, flip=flip, **bias, **epilogue)

    def features_to_image(self, thin: bool, big, out, out_pitch: int, name: str, h: int, w: int, cs: int, big_ch: int, first: bool, flip: bool = False,
                          key=None):
        return features_to_image(self.dtc, thin, _view(big), out, out_pitch, self.P(name + ".weight"), self.Wp(key or ("b" if flip else "f", name)),
                                 self.N, h, w, cs, big_ch, first, flip=flip, bias=None if flip else self.P(name + ".bias"))

    def image_wgrad(self, thin: bool, image, big, name: str, thin_ws, h: int, w: int, cs: int, big_ch: int, first: bool):
        return image_wgrad(self.dtc, thin, self.wplans, image, big, self.P(name + ".weight"), self.poff(name + ".weight"), self.poff(name + ".bias"),
                           thin_ws, self.N, h, w, cs, big_ch, first)


# ---- fused multi-head self-attention (csrc/attention.hip) ----
ATTN_HEAD_DIMS = (16, 32, 64)


def attn_args(dtype: int, batch: int, seq: int, heads: int, head_dim: int, *, qkv=None, out=None, lse=None, d_out=None, d_qkv=None,
              weights=None, workspace: Optional[torch.Tensor] = None) -> A.AttnArgs:
    """qkv (batch, seq, 3 * heads * head_dim), out / d_out (batch, seq, heads * head_dim) in ``dtype``; lse (batch, heads, seq) and
    weights (batch, seq, seq) fp32; tensors or device addresses, None for what the entry point at hand does not use"""
    a = A.AttnArgs()
    a.dtype, a.batch, a.seq, a.heads, a.head_dim = dtype, batch, seq, heads, head_dim
    a.qkv, a.out, a.lse, a.d_out, a.d_qkv, a.weights = _ptr(qkv), _ptr(out), _ptr(lse), _ptr(d_out), _ptr(d_qkv), _ptr(weights)
    if workspace is not None:
        a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    return a


def attention_workspace_bytes(a: A.AttnArgs) -> int:
    n = int(A.lib().srganfd_attention_workspace_bytes(C.byref(a)))
    if n == 0:
        raise A.SrganfdError("attention_workspace_bytes: " + A.lib().srganfd_last_error().decode())
    return n


def attn_work(a: A.AttnArgs, kind: str):
    """(algorithmic FLOP, algorithmic bytes): 4 B H L^2 D forward (two products), 2 B H L^2 D for the weights, 10 B H L^2 D backward"""
    es, c = esize(a.dtype), a.heads * a.head_dim
    unit = 2.0 * a.batch * a.heads * a.seq * a.seq * a.head_dim
    tok = float(a.batch) * a.seq
    if kind == "fwd":
        return 2 * unit, tok * (4 * c * es + 4 * a.heads)
    if kind == "weights":
        return unit, tok * (2 * c * es + 4 * a.heads + 4 * a.seq)
    return 5 * unit, tok * (8 * c * es + 12 * a.heads)


class Attention(_Bracketed):
    """one call of the fused attention kernels: ``op`` "fwd" | "weights" | "bwd" over ``args`` (attn_args').  Under a PerCall, the
    weights launch writes the pass's own tensor."""
    kind = "attention"

    def __init__(self, op: str, args: A.AttnArgs):
        self.op, self.args = op, args
        self.label, self.work = "attn_%s_kernel<%s,D=%d>" % (op, A.DT_NAME[args.dtype], args.head_dim), attn_work(args, op)

    def set_output(self, ptr: int) -> None:
        self.args.weights = ptr

    def _issue(self, run: Run) -> None:
        A.check(getattr(run.L, "srganfd_attention_" + self.op)(C.byref(self.args), run.st), "attention_" + self.op)


def launch_alone(item, rec=None) -> None:
    """one item on the current stream, outside a launch list (tests, tools)"""
    run = Run(item.kind)
    run.rec = rec
    item.launch(run)


def attention_fwd(a: A.AttnArgs, rec=None) -> None:
    """out = softmax(q k^T / sqrt(D)) v and lse, one launch on the current stream"""
    launch_alone(Attention("fwd", a), rec)


def attention_weights(a: A.AttnArgs, rec=None) -> None:
    """the head-averaged probabilities (nn.MultiheadAttention's second result), a launch of its own"""
    launch_alone(Attention("weights", a), rec)


def attention_bwd(a: A.AttnArgs, rec=None) -> None:
    """d_qkv from qkv, out, lse and d_out: two launches (dq per query block, dk / dv per key block), bit-reproducible"""
    launch_alone(Attention("bwd", a), rec)


# ---- A-ESRGAN's pixel attention (csrc/pixel_gate.hip): z = x * (1 + sigmoid(a)) and its backward ----
def pixel_gate_args(dtype: int, npix: int, c: int, x: A.View, a: A.View, *, z: A.View = A.NULL_VIEW, dz: A.View = A.NULL_VIEW,
                    dx: A.View = A.NULL_VIEW, da: A.View = A.NULL_VIEW) -> tuple:
    """srganfd_pixel_gate's arguments without the stream: the forward with ``z``, the backward with ``dz``, ``dx`` and ``da`` (``da``
    may be ``dz`` itself: written in place)"""
    bwd = 1 if dz.ptr else 0
    return (bwd, x, a, dz if bwd else z, dx, da, dtype, npix, c)


class PixelGate(_Bracketed):
    """one srganfd_pixel_gate launch (``args``: pixel_gate_args').  Algorithmic work: bytes only -- x and a read and z written, or
    x, a and dz read and dx and da written, once each."""
    kind = "pixel_gate"

    def __init__(self, args: tuple):
        self.args = args
        bwd, dtype, npix, c = args[0], args[6], args[7], args[8]
        self.label = "pixel_gate_%s_kernel<%s>" % ("bwd" if bwd else "fwd", A.DT_NAME[dtype])
        self.work = (0.0, float(npix) * c * esize(dtype) * (5 if bwd else 3))

    def _issue(self, run: Run) -> None:
        A.check(run.L.srganfd_pixel_gate(*self.args, run.st), "pixel_gate(bwd)" if self.args[0] else "pixel_gate")


def pixel_gate(args: tuple, rec=None) -> None:
    """one launch on the current stream, outside a launch list (tests, tools)"""
    launch_alone(PixelGate(args), rec)


# ---- post-norm transformer encoder layer (csrc/layernorm.hip, csrc/attention_seq.hip): what is no 1x1 convolution ----
SEQ_ATTN_MAX_SEQ = 128


def seq_attn_args(dtype: int, seq: int, nseq: int, heads: int, head_dim: int, *, qkv=None, out=None, lse=None, d_out=None, d_qkv=None,
                  keep=None, keep_scale: float = 1.0) -> A.SeqAttnArgs:
    """qkv (seq, nseq, 3 * heads * head_dim), out / d_out (seq, nseq, heads * head_dim) in ``dtype``; lse (nseq, heads, seq) fp32;
    keep (nseq, heads, seq, seq) uint8 or None; tensors or device addresses, None for what the entry point at hand does not use"""
    a = A.SeqAttnArgs()
    a.dtype, a.seq, a.nseq, a.heads, a.head_dim, a.keep_scale = dtype, seq, nseq, heads, head_dim, keep_scale
    a.qkv, a.out, a.lse, a.d_out, a.d_qkv, a.keep = _ptr(qkv), _ptr(out), _ptr(lse), _ptr(d_out), _ptr(d_qkv), _ptr(keep)
    return a


class SeqAttention(_Bracketed):
    """one srganfd_seq_attention_fwd / _bwd launch (``op`` "fwd" | "bwd") over ``args`` (seq_attn_args').  Algorithmic work as
    attn_work's: 4 N H S^2 D forward, 10 backward."""
    kind = "seq_attention"

    def __init__(self, op: str, args: A.SeqAttnArgs):
        self.op, self.args = op, args
        es, c = esize(args.dtype), args.heads * args.head_dim
        unit, tok = 2.0 * args.nseq * args.heads * args.seq * args.seq * args.head_dim, float(args.nseq) * args.seq
        self.label = "seq_attn_%s_kernel<%s,D=%d%s>" % (op, A.DT_NAME[args.dtype], args.head_dim, ",keep" if args.keep else "")
        self.work = (2 * unit, tok * (4 * c * es + 4 * args.heads)) if op == "fwd" else (5 * unit, tok * (8 * c * es + 4 * args.heads))

    def _issue(self, run: Run) -> None:
        A.check(getattr(run.L, "srganfd_seq_attention_" + self.op)(C.byref(self.args), run.st), "seq_attention_" + self.op)


def add_layernorm_workspace_bytes(ntok: int, e: int) -> int:
    n = int(A.lib().srganfd_add_layernorm_workspace_bytes(ntok, e))
    if n == 0:
        raise A.SrganfdError("add_layernorm_workspace_bytes: " + A.lib().srganfd_last_error().decode())
    return n


class AddLayerNorm(_Bracketed):
    """one srganfd_add_layernorm_fwd launch -- ``x``, ``r``, ``z``, ``y`` (ntok, e) in ``dtype``, ``mean`` / ``rstd`` (ntok) fp32,
    ``gamma`` / ``beta``: addresses in the flat parameters, ``keep``: uint8 mask or None -- or, with ``dy``, ``dx`` and ``dr``, its
    backward: dgamma / dbeta go to elements ``dg_off`` / ``db_off`` of the pass's flat gradient through ``ws``, and are skipped by a
    pass with frozen parameters.  Tensors or device addresses.  Algorithmic work: bytes only."""
    kind = "add_layernorm"

    def __init__(self, dtype: int, ntok: int, e: int, *, z, mean, rstd, gamma: int, keep=None, keep_scale: float = 1.0, eps: float = 1e-5,
                 x=None, r=None, y=None, beta: int = 0, dy=None, dx=None, dr=None, dg_off: int = -1, db_off: int = -1,
                 ws: Optional[torch.Tensor] = None):
        self.bwd = dy is not None
        self.dtype, self.ntok, self.e, self.eps, self.keep_scale = dtype, ntok, e, eps, keep_scale
        self.z, self.mean, self.rstd, self.gamma, self.beta, self.keep = _ptr(z), _ptr(mean), _ptr(rstd), gamma, beta, _ptr(keep)
        self.x, self.r, self.y, self.dy, self.dx, self.dr = _ptr(x), _ptr(r), _ptr(y), _ptr(dy), _ptr(dx), _ptr(dr)
        self.dg_off, self.db_off, self.ws = dg_off, db_off, ws
        self.label = "add_layernorm_%s_kernel<%s%s>" % ("bwd" if self.bwd else "fwd", A.DT_NAME[dtype], ",keep" if keep is not None else "")
        self.work = (0.0, float(ntok) * e * (esize(dtype) * 4 + (1 if keep is not None else 0)))

    def _issue(self, run: Run) -> None:
        if not self.bwd:
            A.check(run.L.srganfd_add_layernorm_fwd(self.dtype, self.x, self.r, self.keep, self.keep_scale, self.gamma, self.beta, self.eps, self.z,
                                                    self.y, self.mean, self.rstd, self.ntok, self.e, run.st), "add_layernorm_fwd")
            return
        params = run.need_wgrad and self.dg_off >= 0
        A.check(run.L.srganfd_add_layernorm_bwd(self.dtype, self.dy, self.z, self.mean, self.rstd, self.gamma, self.keep, self.keep_scale, self.dx,
                                                self.dr, run.grad + 4 * self.dg_off if params else None, run.grad + 4 * self.db_off if params else None,
                                                self.ws.data_ptr() if params else None, self.ws.numel() if params else 0, self.ntok, self.e, run.st),
                "add_layernorm_bwd")


class DropoutApply(_Bracketed):
    """one srganfd_dropout_apply launch: y = x * keep * scale over ``numel`` elements (y may be x)"""
    kind = "dropout_apply"

    def __init__(self, dtype: int, x, keep, scale: float, y, numel: int):
        self.args = (dtype, _ptr(x), _ptr(keep), scale, _ptr(y), numel)
        self.label, self.work = "dropout_apply_kernel<%s>" % A.DT_NAME[dtype], (0.0, float(numel) * (2 * esize(dtype) + 1))

    def _issue(self, run: Run) -> None:
        A.check(run.L.srganfd_dropout_apply(*self.args, run.st), "dropout_apply")


# same-box A/B switch (0: one group of launches per layer, the round-1 form); both forms run in the HIP library and agree to the bit
_SN_BATCH = os.environ.get("SRGANFD_SN_BATCH", "1") != "0"


def spectral_norm_batch(layers: Sequence[tuple], training: bool, workspace: torch.Tensor, eps: float = 1e-12) -> None:
    """layers: (w_orig_ptr, u_ptr, v_ptr, rows, cols, sigma_ptr, inv_sigma_ptr); all of them in ceil(n / 8) x 4 launches."""
    if not _SN_BATCH:
        for (w, u, v, rows, cols, sig, isig) in layers:
            A.check(A.lib().srganfd_spectral_norm(w, u, v, rows, cols, 1 if training else 0, eps, sig, isig, workspace.data_ptr(), A.stream_ptr()), "spectral_norm")
        return
    arr = (A.SnJob * len(layers))()
    off, base = 0, workspace.data_ptr()
    for q, (w, u, v, rows, cols, sig, isig) in zip(arr, layers):
        q.w_orig, q.u, q.v, q.sigma_out, q.inv_sigma_out, q.rows, q.cols = w, u, v, sig, isig, rows, cols
        q.workspace = base + 4 * off
        off += A.sn_ws_floats(rows, cols)
    assert off <= workspace.numel() and workspace.dtype == torch.float32
    A.check(A.lib().srganfd_spectral_norm_batch(arr, len(layers), 1 if training else 0, eps, A.stream_ptr()), "spectral_norm_batch")


def spectral_norm_grad_batch(layers: Sequence[tuple], workspace: torch.Tensor, beta: float = 0.0) -> None:
    """layers: (g_weight_ptr, w_orig_ptr, u_ptr, v_ptr, inv_sigma_ptr, dw_orig_ptr, rows, cols)."""
    if not layers:
        return
    if not _SN_BATCH:
        for (g, w, u, v, isig, dw, rows, cols) in layers:
            A.check(A.lib().srganfd_spectral_norm_grad(g, w, u, v, isig, dw, rows, cols, beta, workspace.data_ptr(), A.stream_ptr()), "spectral_norm_grad")
        return
    arr = (A.SnGradJob * len(layers))()
    assert len(layers) * A.SN_GRAD_WS_FLOATS <= workspace.numel() and workspace.dtype == torch.float32
    for i, (q, (g, w, u, v, isig, dw, rows, cols)) in enumerate(zip(arr, layers)):
        q.g_weight, q.w_orig, q.u, q.v, q.inv_sigma, q.dw_orig, q.rows, q.cols = g, w, u, v, isig, dw, rows, cols
        q.workspace = workspace.data_ptr() + 4 * i * A.SN_GRAD_WS_FLOATS
    A.check(A.lib().srganfd_spectral_norm_grad_batch(arr, len(layers), beta, A.stream_ptr()), "spectral_norm_grad_batch")
