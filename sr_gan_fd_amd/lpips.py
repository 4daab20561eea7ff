"""LPIPS v0.1 on AlexNet: the decision metric of the reference's validation loop (``LPIPS(net='alex')`` at train_bsrgan.py:115,
called as ``lpips_model(sr, gt)`` at :571; bsrgan_config.py:65 picks the best checkpoint by it), fp32, forward only, in HIP
(csrc/lpips.hip): five convolution launches over the 2N batch of both inputs (both max-pools are folded into the gather of
the convolution that follows them) and two launches for the head."""
from __future__ import annotations

import ctypes as C
import warnings

import torch
from torch import Tensor, nn

from . import _abi as A

# (torchvision `features` index, cin, cout, ksize, stride, pad, reads through MaxPool(3, 2))
ALEX_CONVS = ((0, 3, 64, 11, 4, 2, False), (3, 64, 192, 5, 1, 2, True), (6, 192, 384, 3, 1, 1, True),
              (8, 384, 256, 3, 1, 1, False), (10, 256, 256, 3, 1, 1, False))
CHANNELS = tuple(c[2] for c in ALEX_CONVS)
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
MIN_SIZE = 31       # tap 1 must be 7 x 7 for the second pool to see a 3 x 3 map: (31 + 4 - 11) // 4 + 1 = 7

_warned = False


def map_sizes(h: int, w: int):
    """[(h_k, w_k)] of the five taps of an h x w input (pools floor, no padding)"""
    if h < MIN_SIZE or w < MIN_SIZE:
        raise A.SrganfdError(f"LPIPS: a {h} x {w} image is too small: H and W must be at least {MIN_SIZE} (AlexNet's second 3 x 3 "
                             "max-pool needs a 7 x 7 first feature map)")
    t1 = ((h + 4 - 11) // 4 + 1, (w + 4 - 11) // 4 + 1)
    t2 = ((t1[0] - 3) // 2 + 1, (t1[1] - 3) // 2 + 1)
    t3 = ((t2[0] - 3) // 2 + 1, (t2[1] - 3) // 2 + 1)
    return [t1, t2, t3, t3, t3]


class ScalingLayer(nn.Module):
    def __init__(self) -> None:
        super().__init__()
        self.register_buffer("shift", torch.tensor(SHIFT)[None, :, None, None])
        self.register_buffer("scale", torch.tensor(SCALE)[None, :, None, None])


class _Holder(nn.Module):
    """a container whose children carry the names the `lpips` package's state dict uses"""

    def __init__(self, children: dict) -> None:
        super().__init__()
        for name, m in children.items():
            self.add_module(name, m)


class LPIPS(nn.Module):
    """Same constructor and call as the `lpips` package's ``LPIPS`` for what the reference uses: ``LPIPS(net='alex')``, version
    0.1, linear layers on, ``spatial=False``, eval mode.  Anything else raises ``SrganfdError``.  ``forward(in0, in1)`` takes two
    (N,3,H,W) fp32 GPU tensors (H, W >= 31; slices and other non-contiguous views are read in place) and returns the distance as
    an (N,1,1,1) fp32 tensor on the device, detached; nothing is read back to the host.  ``normalize=True`` maps [0,1] inputs to
    [-1,1] first; the reference's scripts leave it False, so that is the default.

    Weights.  Nothing is ever downloaded.  ``model_path`` is the package's linear-layer file (keys ``lin{k}.model.1.weight``,
    (1,C_k,1,1)); ``backbone_weights_path`` is a torchvision ``alexnet`` state dict (``features.{0,3,6,8,10}.{weight,bias}``,
    with or without a ``"state_dict"`` wrapper).  ``state_dict()`` / ``load_state_dict()`` use the package's module layout --
    ``scaling_layer.shift/scale``, ``net.slice1.0.*``, ``net.slice2.3.*``, ``net.slice3.6.*``, ``net.slice4.8.*``,
    ``net.slice5.10.*``, ``lin{k}.model.1.weight``, with ``lins.{k}.model.1.weight`` accepted as an alias -- so a state dict saved
    where the package is installed loads here.  That key layout is written from memory of the package, which is on none of this
    project's machines; parity with the published ``alex.pth`` / torchvision weights is therefore not pinned by a test, the
    arithmetic is (tests/test_lpips_gpu.py, synthetic weights against an fp64 restatement).  Without weight files the module
    uses a seeded initialisation (He-initialised convolutions, zero biases, non-negative linear weights) and warns once: such
    values are reproducible but are not the published metric."""

    def __init__(self, pretrained: bool = True, net: str = "alex", version: str = "0.1", lpips: bool = True, spatial: bool = False,
                 pnet_rand: bool = False, pnet_tune: bool = False, use_dropout: bool = True, model_path: str | None = None,
                 backbone_weights_path: str | None = None, eval_mode: bool = True, verbose: bool = True, seed: int = 0) -> None:
        super().__init__()
        supported = "supported: net='alex', version='0.1', lpips=True, spatial=False"
        if net not in ("alex", "alexnet"):
            raise A.SrganfdError(f"LPIPS: net={net!r} has no HIP path ({supported})")
        if str(version) != "0.1":
            raise A.SrganfdError(f"LPIPS: version={version!r} is not implemented ({supported})")
        if not lpips:
            raise A.SrganfdError(f"LPIPS: lpips=False (no linear layers) is not implemented ({supported})")
        if spatial:
            raise A.SrganfdError(f"LPIPS: spatial=True (a distance map) is not implemented ({supported})")
        self.pnet_type, self.version, self.lpips, self.spatial = "alex", "0.1", True, False
        self.chns = list(CHANNELS)
        self.L = len(CHANNELS)
        self.scaling_layer = ScalingLayer()
        self.net = _Holder({f"slice{k + 1}": _Holder({str(idx): nn.Conv2d(cin, cout, ks, st, pd)})
                            for k, (idx, cin, cout, ks, st, pd, _) in enumerate(ALEX_CONVS)})
        for k, c in enumerate(CHANNELS):
            self.add_module(f"lin{k}", _Holder({"model": _Holder({"1": nn.Conv2d(c, 1, 1, bias=False)})}))
        self._seeded_init(seed)
        if backbone_weights_path:
            self._load_backbone(backbone_weights_path)
        if model_path:
            self._load_lins(model_path)
        global _warned
        if not (backbone_weights_path and model_path) and not _warned:
            _warned = True
            missing = " and ".join(n for n, p in (("backbone_weights_path", backbone_weights_path), ("model_path", model_path)) if not p)
            warnings.warn(f"LPIPS: no {missing} given: the missing weights are a seeded initialisation. The values are reproducible but "
                          "are NOT the published LPIPS metric; nothing is downloaded.", stacklevel=2)
        for p in self.parameters():
            p.requires_grad_(False)
        self._packed = None          # (key, tensors): weights in the kernels' layout, once per device and weight version
        self._ws = {}                # (device, n, h, w) -> workspace; a few sizes are kept (validation images vary)
        if eval_mode:
            self.eval()

    # ---- weights ----
    def _convs(self):
        return [getattr(getattr(self.net, f"slice{k + 1}"), str(c[0])) for k, c in enumerate(ALEX_CONVS)]

    def _lins(self):
        return [getattr(self, f"lin{k}").model._modules["1"] for k in range(self.L)]

    def _seeded_init(self, seed: int) -> None:
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for conv in self._convs():
                fan_in = conv.weight[0].numel()
                conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
                conv.bias.zero_()
            for lin in self._lins():
                lin.weight.copy_(torch.rand(lin.weight.shape, generator=g) / lin.weight.shape[1])

    def _load_backbone(self, path: str) -> None:
        try:
            sd = torch.load(path, map_location="cpu")
        except (OSError, RuntimeError, ValueError) as e:
            raise A.SrganfdError(f"LPIPS: cannot read the backbone weights {path!r}: {e}") from e
        sd = sd.get("state_dict", sd)
        with torch.no_grad():
            for conv, c in zip(self._convs(), ALEX_CONVS):
                for part in ("weight", "bias"):
                    key = f"features.{c[0]}.{part}"
                    if key not in sd:
                        raise A.SrganfdError(f"LPIPS: the backbone weights {path!r} have no '{key}' (a torchvision alexnet state dict is needed)")
                    dst = getattr(conv, part)
                    if tuple(sd[key].shape) != tuple(dst.shape):
                        raise A.SrganfdError(f"LPIPS: '{key}' of {path!r} has shape {tuple(sd[key].shape)}, need {tuple(dst.shape)}")
                    dst.copy_(sd[key])
        self._packed = None

    def _load_lins(self, path: str) -> None:
        try:
            sd = torch.load(path, map_location="cpu")
        except (OSError, RuntimeError, ValueError) as e:
            raise A.SrganfdError(f"LPIPS: cannot read the linear layers {path!r}: {e}") from e
        sd = self._fold_aliases(sd.get("state_dict", sd))
        with torch.no_grad():
            for k, lin in enumerate(self._lins()):
                key = f"lin{k}.model.1.weight"
                if key not in sd:
                    raise A.SrganfdError(f"LPIPS: the linear-layer file {path!r} has no '{key}'")
                if tuple(sd[key].shape) != tuple(lin.weight.shape):
                    raise A.SrganfdError(f"LPIPS: '{key}' of {path!r} has shape {tuple(sd[key].shape)}, need {tuple(lin.weight.shape)}")
                lin.weight.copy_(sd[key])
        self._packed = None

    @staticmethod
    def _fold_aliases(sd):
        """``lins.{k}.*`` (the package's ModuleList over the same layers) -> ``lin{k}.*``; a duplicate must agree"""
        out = {}
        for key, v in sd.items():
            if not key.startswith("lins."):
                out[key] = v
        for key, v in sd.items():
            if key.startswith("lins."):
                k, rest = key[len("lins."):].split(".", 1)
                own = f"lin{k}.{rest}"
                if own in out:
                    if out[own].shape != v.shape or not torch.equal(out[own].to(v.device), v):
                        raise A.SrganfdError(f"LPIPS: '{key}' and '{own}' name the same layer but hold different values")
                else:
                    out[own] = v
        return out

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        self._packed = None
        return super().load_state_dict(self._fold_aliases(state_dict), strict=strict, **kw)

    def _apply(self, fn, *args, **kw):
        self._packed = None
        return super()._apply(fn, *args, **kw)

    def _on(self, device):
        """the kernels' operands on `device`, packed once: per conv ([K][cout] weights, bias), the five lin vectors"""
        params = [p for c in self._convs() for p in (c.weight, c.bias)] + [l.weight for l in self._lins()]
        key = (device, tuple((p.data_ptr(), p._version) for p in params))
        if self._packed is None or self._packed[0] != key:
            # the scaling layer's six constants travel as kernel arguments: read once here (load_state_dict / .to() reset the cache)
            shift, scale = tuple(self.scaling_layer.shift.flatten().tolist()), tuple(self.scaling_layer.scale.flatten().tolist())
            with torch.no_grad():
                convs = []
                for conv, c in zip(self._convs(), ALEX_CONVS):
                    w = conv.weight.detach().to(device=device, dtype=torch.float32)
                    # first conv: rows in (c, ky, kx) order, as the NCHW gather walks them; the others (ky, kx, c): NHWC chunks
                    w = w.reshape(c[2], -1).t() if c[0] == 0 else w.permute(2, 3, 1, 0).reshape(-1, c[2])
                    convs.append((w.contiguous(), conv.bias.detach().to(device=device, dtype=torch.float32).contiguous()))
                lins = [l.weight.detach().to(device=device, dtype=torch.float32).reshape(-1).contiguous() for l in self._lins()]
            self._packed = (key, convs, lins, shift, scale)
        return self._packed[1:]

    def _workspace(self, device, n: int, h: int, w: int) -> Tensor:
        k = (device, n, h, w)
        ws = self._ws.get(k)
        if ws is None:
            nbytes = int(A.lib().srganfd_lpips_workspace_bytes(n, h, w))
            if nbytes < 0:
                A.check(-1, "lpips_workspace_bytes")
            if len(self._ws) >= 8:                       # validation sets mix a few sizes; do not keep one buffer per image ever seen
                self._ws.pop(next(iter(self._ws)))
            ws = self._ws[k] = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
        return ws

    # ---- forward ----
    @staticmethod
    def _check(in0: Tensor, in1: Tensor):
        if in0.dim() != 4 or in1.dim() != 4:
            raise A.SrganfdError(f"LPIPS: needs two (N,3,H,W) tensors, got shapes {tuple(in0.shape)} and {tuple(in1.shape)}")
        if in0.shape != in1.shape:
            raise A.SrganfdError(f"LPIPS: the two inputs differ in shape: {tuple(in0.shape)} and {tuple(in1.shape)}")
        n, c, h, w = in0.shape
        if c != 3:
            raise A.SrganfdError(f"LPIPS: needs 3-channel RGB inputs, have {c} channels")
        if n < 1:
            raise A.SrganfdError("LPIPS: empty batch")
        sizes = map_sizes(h, w)
        if not (in0.is_cuda and in1.is_cuda) or in0.device != in1.device:
            raise A.SrganfdError("LPIPS: both tensors must be on the GPU, on one device (the HIP library is the product; no CPU fallback)")
        return n, h, w, sizes

    def _run(self, in0: Tensor, in1: Tensor, normalize: bool):
        n, h, w, sizes = self._check(in0, in1)
        a, b = in0.detach(), in1.detach()
        if a.dtype != torch.float32:
            a = a.float()
        if b.dtype != torch.float32:
            b = b.float()
        dev = a.device
        convs, lins, shift, scale = self._on(dev)
        ws = self._workspace(dev, n, h, w)
        L, stream = A.lib(), A.stream_ptr()
        maps, off = [], 0
        for (hk, wk), ck in zip(sizes, CHANNELS):
            maps.append(ws[off:off + 2 * n * hk * wk * ck].view(2 * n, hk, wk, ck))
            off += 2 * n * hk * wk * ck
        hin, win = h, w
        for k, (idx, cin, cout, ks, st, pd, pool) in enumerate(ALEX_CONVS):
            ca = A.LpipsConvArgs()
            ca.n, ca.h_in, ca.w_in, ca.cin, ca.cout, ca.ksize, ca.stride, ca.pad = 2 * n, hin, win, cin, cout, ks, st, pd
            ca.pool, ca.first, ca.normalize = int(pool), int(k == 0), int(bool(normalize))
            ca.h_out, ca.w_out = sizes[k]
            if k == 0:
                ca.in0, ca.in1 = a.data_ptr(), b.data_ptr()
                ca.stride0, ca.stride1 = (C.c_int64 * 4)(*a.stride()), (C.c_int64 * 4)(*b.stride())
                ca.shift, ca.scale = (C.c_float * 3)(*shift), (C.c_float * 3)(*scale)
            else:
                ca.x = maps[k - 1].data_ptr()
            ca.w, ca.bias, ca.y = convs[k][0].data_ptr(), convs[k][1].data_ptr(), maps[k].data_ptr()
            A.check(L.srganfd_lpips_conv(C.byref(ca), stream), f"lpips_conv (features.{idx})")
            hin, win = sizes[k]
        taps = (A.LpipsTap * self.L)()
        for k in range(self.L):
            taps[k].maps, taps[k].lin = maps[k].data_ptr(), lins[k].data_ptr()
            taps[k].h, taps[k].w, taps[k].c = sizes[k][0], sizes[k][1], CHANNELS[k]
        out = torch.empty(self.L + 1, n, dtype=torch.float32, device=dev)
        A.check(L.srganfd_lpips_head(taps, self.L, n, out.data_ptr(), ws[off:].data_ptr(), stream), "lpips_head")
        return out, maps

    def forward(self, in0: Tensor, in1: Tensor, retPerLayer: bool = False, normalize: bool = False):
        out, _ = self._run(in0, in1, normalize)
        n = out.shape[1]
        val = out[self.L].view(n, 1, 1, 1)
        if retPerLayer:
            return val, [out[k].view(n, 1, 1, 1) for k in range(self.L)]
        return val

    def features(self, in0: Tensor, in1: Tensor, normalize: bool = False):
        """the five tap maps as (2N, h_k, w_k, C_k) fp32 NHWC tensors (in0's images first), copied out of the workspace: what a
        test compares layer by layer"""
        _, maps = self._run(in0, in1, normalize)
        return [m.clone() for m in maps]
