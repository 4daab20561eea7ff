"""Device-side mirror of the data-side helpers the train loops call on GPU tensors (reference: BSRGAN/imgproc.py for
``random_crop``; Real_ESRGAN/imgproc.py for the on-device degradation stages -- SURVEY 8f N4: ``filter2d_torch``,
``USMSharp``, ``DiffJPEG``, the noise stages, ``degradation_process``; BSRGAN/imgproc.py:492-562 for the blind degradation,
``degradation_process_bsrgan``, with its real JPEG round trip and fp64 blur; Real_ESRGAN/dataset.py:64-133 with imgproc.py:228-606 for
the per-image filter kernels, ``realesrgan_kernel_draws`` / ``blur_kernel_bank`` / ``realesrgan_blur_kernels``).  The cv2 image I/O of that
file stays the reference's own."""
from __future__ import annotations

import math
import random
from typing import Tuple, Union

import numpy as np
import torch
from torch import Tensor, nn

from . import _abi as A


def random_crop(gt_tensor: Tensor, lr_tensor: Tensor, gt_image_size: int, upscale_factor: int) -> Tuple[Tensor, Tensor]:
    """imgproc.random_crop (BSRGAN/imgproc.py:846-886): one (top, left) for the whole batch drawn from Python's
    ``random`` stream (row first, then column -- seed per rank under data parallelism), LR window at the
    integer-divided position, outputs in ``lr_tensor.dtype``.  The reference copies B slices in a Python loop; here
    each tensor is one strided-copy launch.  Identity-sized requests return the inputs' data unchanged."""
    h, w = gt_tensor.shape[2], gt_tensor.shape[3]
    top = random.randint(0, h - gt_image_size)
    left = random.randint(0, w - gt_image_size)
    lr_top, lr_left, lr_size = top // upscale_factor, left // upscale_factor, gt_image_size // upscale_factor
    if not (gt_tensor.is_cuda and lr_tensor.is_cuda):
        raise A.SrganfdError("random_crop: tensors must be on the GPU (the HIP library is the product; no CPU fallback)")
    L, st = A.lib(), A.stream_ptr()
    out = []
    for src, t, l, s in ((gt_tensor, top, left, gt_image_size), (lr_tensor, lr_top, lr_left, lr_size)):
        x = src.contiguous().float()
        dst = torch.empty(x.shape[0], x.shape[1], s, s, dtype=torch.float32, device=x.device)
        A.check(L.srganfd_crop_nchw(x.data_ptr(), dst.data_ptr(), x.shape[0], x.shape[1], x.shape[2], x.shape[3], t, l, s, s, st), "crop_nchw")
        out.append(dst.to(lr_tensor.dtype))
    return out[0], out[1]


def image_to_tensor_u8(images_u8: Tensor, top: int = 0, left: int = 0, size=None, bgr: bool = True, range_norm: bool = False) -> Tensor:
    """The reference's per-image host ingest for a whole batch on the device: ``cv2.imread(...).astype(np.float32) / 255.``
    (dataset.py:66), the crop window, ``cv2.cvtColor(..., COLOR_BGR2RGB)`` (:81) and ``image_to_tensor(image, range_norm, False)``
    (imgproc.py:331-358: HWC -> CHW, optional [0, 1] -> [-1, 1]) in one kernel.  ``images_u8``: (N, H, W, 3) uint8 on the GPU, as decoded
    (BGR when ``bgr``); returns (N, 3, h, w) fp32.  The batch crosses PCIe as bytes -- a quarter of the fp32 tensors the reference copies."""
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[-1] != 3:
        raise A.SrganfdError("image_to_tensor_u8 takes (N, H, W, 3) uint8 images")
    _need_gpu(images_u8, "image_to_tensor_u8")
    n, h, w, _ = images_u8.shape
    ph, pw = (h - top, w - left) if size is None else ((size, size) if isinstance(size, int) else tuple(size))
    src = images_u8.contiguous()
    out = torch.empty(n, 3, ph, pw, dtype=torch.float32, device=src.device)
    A.check(A.lib().srganfd_u8hwc_to_nchw(src.data_ptr(), out.data_ptr(), n, h, w, top, left, ph, pw, 1 if bgr else 0, 255.0, A.stream_ptr()), "u8hwc_to_nchw")
    return out.mul_(2.0).sub_(1.0) if range_norm else out


def _need_gpu(t: Tensor, what: str) -> None:
    if not t.is_cuda:
        raise A.SrganfdError(f"{what}: tensors must be on the GPU (the HIP library is the product; no CPU fallback)")


# ---- MATLAB imresize (ESRGAN/imgproc.py:34-127, 202-288; the same text in every imgproc.py of the reference) --------------------
def _cubic_f32(x: Tensor) -> Tensor:
    """Keys' cubic with a = -0.5 on a float32 tensor: the two polynomial pieces, each masked by its interval"""
    ax = torch.abs(x)
    ax2, ax3 = ax ** 2, ax ** 3
    inner = (1.5 * ax3 - 2.5 * ax2 + 1) * (ax <= 1).type_as(ax)
    outer = (-0.5 * ax3 + 2.5 * ax2 - 4 * ax + 2) * ((ax > 1) * (ax <= 2)).type_as(ax)
    return inner + outer


def _resize_tables_host(in_length: int, out_length: int, scale: float, antialiasing: bool):
    """Weights and first source indices of one side, as ``_calculate_weights_indices`` (imgproc.py:53-127) makes them: computed in
    FLOAT32 with torch's CPU ops in the reference's order of operations (output coordinates, their inverse map, the left-most
    contributing sample, the kernel -- stretched and scaled when it shrinks with antialiasing -- and the row normalisation), so the
    weights carry the reference's bits; fp64 tables would differ from it by up to 3.6e-6 in the result at scales like 0.3 or 3.0.
    Returns ``(weights (out, taps) float32, first (out,) int32, pad_start, pad_end)``: ``first`` is the 0-based source index of tap 0
    (negative / past the end where the symmetric padding is read), ``pad_*`` the reference's ``sym_len_s`` / ``sym_len_e``.  The
    edge columns are dropped exactly where the reference drops them (it drops the outermost pair whenever the first column holds a
    zero, which it always does: that sample lies half a kernel width or more from the centre)."""
    width = 4.0
    shrink = scale < 1 and antialiasing
    if shrink:
        width = width / scale
    x = torch.linspace(1, out_length, out_length)
    u = x / scale + 0.5 * (1 - 1 / scale)
    left = torch.floor(u - width / 2)
    p = math.ceil(width) + 2
    idx = left.view(out_length, 1) + torch.linspace(0, p - 1, p).view(1, p)          # 1-based sample numbers, float32 (exact)
    dist = u.view(out_length, 1) - idx
    w = scale * _cubic_f32(dist * scale) if shrink else _cubic_f32(dist)
    w = w / torch.sum(w, 1).view(out_length, 1)
    zeros = torch.sum(w == 0, 0)
    if int(zeros[0]) != 0:
        idx, w = idx[:, 1:p - 1], w[:, 1:p - 1]
    if int(zeros[-1]) != 0:
        idx, w = idx[:, :p - 2], w[:, :p - 2]
    pad_start = int(-idx.min() + 1)
    pad_end = int(idx.max() - in_length)
    first = (idx[:, 0] - 1).to(torch.int32)
    return w.contiguous(), first.contiguous(), pad_start, pad_end


_RESIZE_TABLES = {}          # (in, out, scale, antialiasing) -> host tables; (..., device) -> their device copies.  Never evicted: a
                             # training run resizes a handful of lengths, and a copy freed here could still be read by a launch in flight


def _resize_tables(in_length: int, out_length: int, scale: float, antialiasing: bool, side: str, device=None):
    """one side's tables, cached: on the host (``device`` None), where the reference's failure on padding longer than the image becomes
    a ValueError, or as device copies ``(weights, first, taps)``"""
    key = (in_length, out_length, float(scale), bool(antialiasing))
    host = _RESIZE_TABLES.get(key)
    if host is None:
        host = _RESIZE_TABLES[key] = _resize_tables_host(in_length, out_length, scale, antialiasing)
    if max(host[2], host[3]) > in_length:
        raise ValueError(f"image_resize: the {side} of {in_length} pixels is shorter than the symmetric padding the kernel needs "
                         f"({host[2]} before, {host[3]} after) at scale {scale}")
    if device is None:
        return host
    dev = _RESIZE_TABLES.get(key + (str(device),))
    if dev is None:
        dev = _RESIZE_TABLES[key + (str(device),)] = (host[0].to(device), host[1].to(device), host[0].shape[1])
    return dev


def image_resize(image: Tensor, scale_factor: float, antialiasing: bool = True) -> Tensor:
    """imgproc.image_resize (ESRGAN/imgproc.py:202-288; dataset.py:73 makes every LR image with it): MATLAB's ``imresize`` -- cubic
    a = -0.5, widened by 1 / scale when it shrinks with ``antialiasing``, symmetric padding, rows then columns, float32.  ``image``:
    a GPU tensor ``(H, W)`` or ``(C, H, W)`` (the reference's forms) or a batch ``(N, C, H, W)``; returns float32 of the same rank,
    ``math.ceil(in * scale_factor)`` per side.  One HIP launch for the whole batch (srganfd_imresize) instead of the reference's
    Python loop over output rows and columns; no autograd (the reference calls it on data).  CPU tensors and numpy arrays raise
    ``SrganfdError``; ``scale_factor <= 0`` raises ``ValueError``.  Differences from the reference, both where it cannot run as
    written: a side shorter than its padding (4 x 4 at 1/4 needs 7 rows) raises ``ValueError`` naming the side before anything is
    launched (the reference dies in a ``copy_`` size mismatch), and a side that needs no padding at its end (64 x 64 at 1/4 without
    antialiasing: ``image[:, -0:, :]`` is the whole image there and the reference raises) returns the defined result -- there is
    nothing to reflect on that side."""
    if not torch.is_tensor(image):
        raise A.SrganfdError("image_resize: takes GPU tensors (the HIP library is the product; no CPU fallback)")
    if image.dim() not in (2, 3, 4):
        raise A.SrganfdError("image_resize takes (H, W), (C, H, W) or (N, C, H, W) tensors")
    if not scale_factor > 0:
        raise ValueError(f"image_resize: scale_factor must be positive, got {scale_factor}")
    h, w = image.shape[-2:]
    oh, ow = math.ceil(h * scale_factor), math.ceil(w * scale_factor)
    for args in ((h, oh, "height"), (w, ow, "width")):             # the argument errors come first, whatever the device
        _resize_tables(args[0], args[1], scale_factor, antialiasing, args[2])
    _need_gpu(image, "image_resize")
    wt_h, first_h, taps_h = _resize_tables(h, oh, scale_factor, antialiasing, "height", image.device)
    wt_w, first_w, taps_w = _resize_tables(w, ow, scale_factor, antialiasing, "width", image.device)
    x = image.detach().contiguous().float()
    out = torch.empty(*x.shape[:-2], oh, ow, dtype=torch.float32, device=x.device)
    A.check(A.lib().srganfd_imresize(x.data_ptr(), x.numel() // (h * w), h, w, oh, ow, wt_h.data_ptr(), first_h.data_ptr(), taps_h,
                                     wt_w.data_ptr(), first_w.data_ptr(), taps_w, out.data_ptr(), A.stream_ptr()), "imresize")
    return out


def filter2d_torch(image: Tensor, kernel: Tensor) -> Tensor:
    """imgproc.filter2d_torch (Real_ESRGAN/imgproc.py:1092-1124): reflect padding + per-image (or shared) k x k
    cross-correlation of every channel.  One LDS-tiled HIP launch instead of pad + view + grouped conv2d; an even
    kernel size raises ``ValueError("Wrong kernel size.")`` like the reference."""
    k = kernel.size(-1)
    b, c, h, w = image.size()
    if k % 2 != 1:
        raise ValueError("Wrong kernel size.")
    _need_gpu(image, "filter2d_torch")
    x = image.detach().contiguous().float()
    kk = kernel.detach().to(device=x.device, dtype=torch.float32).contiguous()
    out = torch.empty_like(x)
    A.check(A.lib().srganfd_filter2d(x.data_ptr(), kk.data_ptr(), 1 if kk.size(0) == 1 else kk.size(0), b, c, h, w, k, out.data_ptr(),
                                     A.stream_ptr()), "filter2d")
    return out


def _gaussian_kernel_1d(ksize: int, sigma: float) -> np.ndarray:
    """what cv2.getGaussianKernel(ksize, sigma) returns per OpenCV's documentation (OpenCV is not a dependency here)"""
    if sigma <= 0:
        sigma = 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) * 0.5
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return (g / g.sum()).reshape(ksize, 1)


class USMSharp(nn.Module):
    """imgproc.USMSharp (Real_ESRGAN/imgproc.py:1517-1540): same constructor, ``kernel`` buffer (1, r, r) and
    ``forward(x, weight, threshold)``.  Two fused HIP passes: blur -> residual + threshold mask, then blurred mask ->
    blend (the reference runs two grouped convs and six elementwise ops)."""

    def __init__(self, radius: int = 50, sigma: int = 0) -> None:
        super().__init__()
        if radius % 2 == 0:
            radius += 1
        self.radius = radius
        kernel = _gaussian_kernel_1d(radius, sigma)
        kernel = torch.FloatTensor(np.dot(kernel, kernel.transpose())).unsqueeze_(0)
        self.register_buffer("kernel", kernel)

    def _taps(self, device) -> Tuple[Tensor, int]:
        """(filter operand, separable flag).  The constructor's kernel is an outer product, so the two passes run as a
        horizontal + a vertical 1-D filter (2k instead of k*k multiply-adds per pixel); a ``kernel`` buffer that was replaced
        by something of higher rank is detected (checked once per buffer version) and run as the full 2-D filter."""
        key = (self.kernel.data_ptr(), self.kernel._version, str(device))
        if getattr(self, "_taps_key", None) != key:
            k2 = self.kernel.detach().double().cpu().reshape(self.radius, self.radius)
            mid = self.radius // 2
            sep = None
            if float(k2[mid, mid]) != 0.0:
                col, row = k2[:, mid] / k2[mid, mid], k2[mid, :]
                if float((torch.outer(col, row) - k2).abs().max()) <= 1e-6 * float(k2.abs().max()):    # fp32 rounding of the stored outer product is ~2e-7
                    sep = torch.cat([col, row]).float()
            self._taps_cache = ((sep, 1) if sep is not None else (self.kernel.detach().float().contiguous(), 0))
            self._taps_cache = (self._taps_cache[0].to(device), self._taps_cache[1])
            self._taps_key = key
        return self._taps_cache

    def forward(self, x: Tensor, weight: float, threshold: int) -> Tensor:
        _need_gpu(x, "USMSharp")
        xx = x.detach().contiguous().float()
        b, c, h, w = xx.shape
        kk, separable = self._taps(xx.device)
        out = torch.empty_like(xx)
        ws = torch.empty(2 * xx.numel(), dtype=torch.float32, device=xx.device)
        A.check(A.lib().srganfd_usm_sharp(xx.data_ptr(), kk.data_ptr(), separable, b, c, h, w, self.radius, float(weight), float(threshold),
                                          out.data_ptr(), ws.data_ptr(), A.stream_ptr()), "usm_sharp")
        return out


class DiffJPEG(nn.Module):
    """imgproc.DiffJPEG (Real_ESRGAN/imgproc.py:1465-1497): ``forward(x, quality)`` with ``quality`` an int / float or a
    per-image tensor, which -- as in the reference (:1476-1480) -- is converted to the compression factor IN PLACE.
    The whole round trip (colour transform, 4:2:0, DCT, quantise, round, inverse) is one HIP kernel, one wavefront per
    16x16 MCU.  Forward only: the reference trains with ``DiffJPEG()`` inside ``torch.no_grad`` data preparation."""

    def __init__(self, differentiable: bool = False) -> None:
        super().__init__()
        self.differentiable = differentiable
        L = A.lib()
        t = np.zeros(L.srganfd_diff_jpeg_table_floats(), dtype=np.float32)
        A.check(L.srganfd_diff_jpeg_tables(t.ctypes.data), "diff_jpeg_tables")
        self.register_buffer("tables", torch.from_numpy(t), persistent=False)

    def forward(self, x: Tensor, quality: Union[int, float, Tensor]) -> Tensor:
        _need_gpu(x, "DiffJPEG")
        xx = x.detach().contiguous().float()
        b, c, h, w = xx.shape
        if isinstance(quality, (int, float)):
            q = 5000. / quality if quality < 50 else 200. - quality * 2
            fac, is_factor = torch.full((b,), q / 100., dtype=torch.float32, device=xx.device), 1
        else:
            if quality.dtype != torch.float32 or not quality.is_cuda or not quality.is_contiguous() or quality.numel() != b:
                raise A.SrganfdError("DiffJPEG: quality tensor must be a contiguous float32 GPU tensor with one entry per image")
            fac, is_factor = quality, 0
        tables = self.tables if self.tables.device == xx.device else self.tables.to(xx.device)
        out = torch.empty_like(xx)
        A.check(A.lib().srganfd_diff_jpeg(xx.data_ptr(), b, c, h, w, fac.data_ptr(), is_factor, 1 if self.differentiable else 0,
                                          tables.data_ptr(), out.data_ptr(), A.stream_ptr()), "diff_jpeg")
        return out


_RESIZE_MODES = {"area": 0, "bilinear": 1, "bicubic": 2}

# Where the random draws of the noise / JPEG-quality stages are made.  None: on the image's device (the reference's
# behaviour on a GPU).  "cpu": drawn from torch's CPU generator and copied over -- a run seeded with torch.manual_seed then
# consumes exactly the stream the reference consumes when it runs on the CPU (parity tests, device-independent replays).
DRAW_DEVICE = None


def _draw(fn, *shape, device):
    return fn(*shape, dtype=torch.float32, device=DRAW_DEVICE or device).to(device)


def _poisson(rate: Tensor) -> Tensor:
    return torch.poisson(rate.to(DRAW_DEVICE)).to(rate.device) if DRAW_DEVICE else torch.poisson(rate)


def interpolate(x: Tensor, size=None, scale_factor=None, mode: str = "bilinear") -> Tensor:
    """``torch.nn.functional.interpolate`` as degradation_process calls it (Real_ESRGAN/imgproc.py:2374, :2415-2418,
    :2440-2442, :2454-2456): modes "area" / "bilinear" / "bicubic", align_corners unset; ``scale_factor=`` sizes the output
    as floor(in * scale) and maps coordinates with 1 / scale_factor, ``size=`` with in / out -- torch's rules."""
    _need_gpu(x, "interpolate")
    if mode not in _RESIZE_MODES:
        raise ValueError(f"interpolate: mode {mode!r} is not one of {sorted(_RESIZE_MODES)}")
    if (size is None) == (scale_factor is None):
        raise ValueError("only one of size or scale_factor should be defined")
    xx = x.detach().contiguous().float()
    b, c, h, w = xx.shape
    if size is not None:
        oh, ow = (size, size) if isinstance(size, int) else size
        rs_h = rs_w = 0.0
    else:
        sf = (scale_factor, scale_factor) if isinstance(scale_factor, (int, float)) else tuple(scale_factor)
        oh, ow = int(np.floor(float(h * sf[0]))), int(np.floor(float(w * sf[1])))
        rs_h, rs_w = float(np.float32(1.0 / sf[0])), float(np.float32(1.0 / sf[1]))
    out = torch.empty(b, c, int(oh), int(ow), dtype=torch.float32, device=xx.device)
    A.check(A.lib().srganfd_resize(xx.data_ptr(), b * c, h, w, int(oh), int(ow), _RESIZE_MODES[mode], rs_h, rs_w, out.data_ptr(), A.stream_ptr()), "resize")
    return out


def _per_image(v, b: int, device) -> Tensor:
    if isinstance(v, (float, int)):
        return torch.full((b,), float(v), dtype=torch.float32, device=device)
    return v.detach().to(device=device, dtype=torch.float32).reshape(b).contiguous()


def _add_gaussian_noise_torch(image: Tensor, sigma=10.0, clip: bool = True, rounds: bool = False, gray_noise=0) -> Tensor:
    """imgproc._add_gaussian_noise_torch (Real_ESRGAN/imgproc.py:970-998 over :832-866): the draws come from torch's
    generator on the image's device in the reference's order (the shared (h, w) grey field first, if any image asks for
    grey noise, then the colour field); scaling, grey / colour mixing, the add and the clip are one HIP pass."""
    _need_gpu(image, "_add_gaussian_noise_torch")
    x = image.detach().contiguous().float()
    b, c, h, w = x.shape
    sg = _per_image(sigma, b, x.device)
    if isinstance(gray_noise, (float, int)):
        cal_gray, gray = gray_noise > 0, _per_image(gray_noise, b, x.device)
    else:
        gray = _per_image(gray_noise, b, x.device)
        cal_gray = bool(torch.sum(gray) > 0)
    n_gray = _draw(torch.randn, h, w, device=x.device) if cal_gray else None
    n_color = _draw(torch.randn, b, c, h, w, device=x.device)
    return gaussian_noise_apply(x, n_color, n_gray, sg, gray, clip, rounds)


def gaussian_noise_apply(image: Tensor, randn_color: Tensor, randn_gray_hw, sigma: Tensor, gray_flag: Tensor, clip: bool, rounds: bool) -> Tensor:
    """the deterministic part of the Gaussian-noise stage on given draws (srganfd_gaussian_noise)"""
    b, c, h, w = image.shape
    out = torch.empty_like(image)
    A.check(A.lib().srganfd_gaussian_noise(image.data_ptr(), randn_color.data_ptr(), randn_gray_hw.data_ptr() if randn_gray_hw is not None else None,
                                           sigma.data_ptr(), gray_flag.data_ptr(), b, c, h, w, int(clip), int(rounds), out.data_ptr(), A.stream_ptr()),
            "gaussian_noise")
    return out


def random_add_gaussian_noise_torch(image: Tensor, sigma_range: tuple = (0, 1.0), gray_prob: int = 0, clip: bool = True, rounds: bool = False) -> Tensor:
    """imgproc.random_add_gaussian_noise_torch (Real_ESRGAN/imgproc.py:1032-1060 over :922-943): per-image sigma and grey
    flag drawn with torch.rand in the reference's order, then ``_add_gaussian_noise_torch``."""
    b = image.size(0)
    sigma = _draw(torch.rand, b, device=image.device) * (sigma_range[1] - sigma_range[0]) + sigma_range[0]
    gray_noise = (_draw(torch.rand, b, device=image.device) < gray_prob).float()
    return _add_gaussian_noise_torch(image, sigma, clip, rounds, gray_noise)


def poisson_noise_prepare(image: Tensor, want_gray: bool):
    """8-bit rounded image (and grey image), and vals = 2^ceil(log2(#distinct levels)) per image (imgproc.py:892-910)"""
    b, c, h, w = image.shape
    img_q = torch.empty_like(image)
    gray_q = torch.empty(b, 1, h, w, dtype=torch.float32, device=image.device) if want_gray else None
    vals = torch.empty(b, dtype=torch.float32, device=image.device)
    vals_gray = torch.empty(b, dtype=torch.float32, device=image.device) if want_gray else None
    ws = torch.empty(b * 512, dtype=torch.int32, device=image.device)
    A.check(A.lib().srganfd_poisson_prepare(image.data_ptr(), b, c, h, w, int(want_gray), img_q.data_ptr(), gray_q.data_ptr() if want_gray else None,
                                            vals.data_ptr(), vals_gray.data_ptr() if want_gray else None, ws.data_ptr(), A.stream_ptr()), "poisson_prepare")
    return img_q, gray_q, vals, vals_gray


def poisson_noise_apply(image, img_q, gray_q, pois, pois_gray, vals, vals_gray, scale, gray_flag, clip: bool, rounds: bool) -> Tensor:
    """the deterministic part of the Poisson-noise stage on given draws (srganfd_poisson_apply)"""
    b, c, h, w = image.shape
    out = torch.empty_like(image)
    P = lambda t: t.data_ptr() if t is not None else None
    A.check(A.lib().srganfd_poisson_apply(image.data_ptr(), img_q.data_ptr(), P(gray_q), pois.data_ptr(), P(pois_gray), vals.data_ptr(), P(vals_gray),
                                          scale.data_ptr(), P(gray_flag), b, c, h, w, int(clip), int(rounds), out.data_ptr(), A.stream_ptr()), "poisson_apply")
    return out


def _add_poisson_noise_torch(image: Tensor, scale=1.0, clip: bool = True, rounds: bool = False, gray_noise=0) -> Tensor:
    """imgproc._add_poisson_noise_torch (Real_ESRGAN/imgproc.py:1001-1029 over :869-919): torch.poisson draws (grey first, as
    in the reference) on rates prepared by one HIP pass, everything after the draws in another."""
    _need_gpu(image, "_add_poisson_noise_torch")
    x = image.detach().contiguous().float()
    b, c, h, w = x.shape
    if isinstance(gray_noise, (float, int)):
        cal_gray, gray = gray_noise > 0, _per_image(gray_noise, b, x.device)
    else:
        gray = _per_image(gray_noise, b, x.device)
        cal_gray = bool(torch.sum(gray) > 0)
    img_q, gray_q, vals, vals_gray = poisson_noise_prepare(x, cal_gray)
    pois_gray = _poisson(gray_q * vals_gray.view(b, 1, 1, 1)) if cal_gray else None
    pois = _poisson(img_q * vals.view(b, 1, 1, 1))
    return poisson_noise_apply(x, img_q, gray_q, pois, pois_gray, vals, vals_gray, _per_image(scale, b, x.device), gray if cal_gray else None, clip, rounds)


def random_add_poisson_noise_torch(image: Tensor, scale_range: tuple = (0, 1.0), gray_prob: int = 0, clip: bool = True, rounds: bool = False) -> Tensor:
    """imgproc.random_add_poisson_noise_torch (Real_ESRGAN/imgproc.py:1063-1089 over :946-967)"""
    b = image.size(0)
    scale = _draw(torch.rand, b, device=image.device) * (scale_range[1] - scale_range[0]) + scale_range[0]
    gray_noise = (_draw(torch.rand, b, device=image.device) < gray_prob).float()
    return _add_poisson_noise_torch(image, scale, clip, rounds, gray_noise)


def quantize_u8(x: Tensor) -> Tensor:
    """clamp(round(x * 255), 0, 255) / 255 -- the last line of degradation_process (Real_ESRGAN/imgproc.py:2460)"""
    _need_gpu(x, "quantize_u8")
    xx = x.detach().contiguous().float()
    out = torch.empty_like(xx)
    A.check(A.lib().srganfd_quantize_u8(xx.data_ptr(), out.data_ptr(), xx.numel(), A.stream_ptr()), "quantize_u8")
    return out


def _jpeg_quality(out: Tensor, jpeg_range) -> Tensor:
    """quality = out.new_zeros(b).uniform_(*range) (imgproc.py:2393-2394)"""
    return torch.zeros(out.size(0), dtype=torch.float32, device=DRAW_DEVICE or out.device).uniform_(*jpeg_range).to(out.device)


def degradation_process(gt: Tensor, gaussian_kernel1: Tensor, gaussian_kernel2: Tensor, sinc_kernel: Tensor, upscale_factor: int,
                        degradation_process_parameters_dict: dict, jpeg_operation: nn.Module = None, usm_sharpener: nn.Module = None):
    """imgproc.degradation_process (Real_ESRGAN/imgproc.py:2323-2462): the second-order degradation of a GT batch on the
    GPU -- [sharpen] blur, random resize, Gaussian-or-Poisson noise, JPEG; blur, resize, noise; then resize + sinc filter
    and JPEG in a random order; 8-bit quantisation.  Host-side draws (numpy / ``random``) are made in the reference's
    order, so a seeded run takes the same branches; every stage is a HIP kernel of this library.  Returns
    ``(gt_usm, gt, lr)``.  Differences from the reference, both where it cannot run as written: the sharpener is called
    as ``usm_sharpener(gt, 0.5, 10)`` (the reference passes no weight / threshold to a forward that requires them;
    0.5 / 10 are its numpy twin's defaults, :1500), and a skipped first blur passes the image on (the reference would hit
    an unbound ``out``; its configs use probability 1.0)."""
    P = degradation_process_parameters_dict
    image_height, image_width = gt.size()[2:4]
    gt_usm = gt
    if usm_sharpener is not None:
        gt_usm = usm_sharpener(gt, 0.5, 10)
    out = gt_usm
    # first degradation: blur, resize, noise, JPEG
    if np.random.uniform() <= P["first_blur_probability"]:
        out = filter2d_torch(gt_usm, gaussian_kernel1)
    updown_type = random.choices(["up", "down", "keep"], P["resize_probability1"])[0]
    if updown_type == "up":
        scale = np.random.uniform(1, P["resize_range1"][1])
    elif updown_type == "down":
        scale = np.random.uniform(P["resize_range1"][0], 1)
    else:
        scale = 1
    mode = random.choice(["area", "bilinear", "bicubic"])
    out = interpolate(out, scale_factor=scale, mode=mode)
    if np.random.uniform() < P["gaussian_noise_probability1"]:
        out = random_add_gaussian_noise_torch(image=out, sigma_range=P["noise_range1"], clip=True, rounds=False, gray_prob=P["gray_noise_probability1"])
    else:
        out = random_add_poisson_noise_torch(image=out, scale_range=P["poisson_scale_range1"], gray_prob=P["gray_noise_probability1"], clip=True,
                                             rounds=False)
    quality = _jpeg_quality(out, P["jpeg_range1"])
    out = jpeg_operation(torch.clamp(out, 0, 1), quality)
    # second degradation: blur, resize, noise
    if np.random.uniform() < P["second_blur_probability"]:
        out = filter2d_torch(out, gaussian_kernel2)
    updown_type = random.choices(["up", "down", "keep"], P["resize_probability2"])[0]
    if updown_type == "up":
        scale = np.random.uniform(1, P["resize_range2"][1])
    elif updown_type == "down":
        scale = np.random.uniform(P["resize_range2"][0], 1)
    else:
        scale = 1
    mode = random.choice(["area", "bilinear", "bicubic"])
    out = interpolate(out, size=(int(image_height / upscale_factor * scale), int(image_width / upscale_factor * scale)), mode=mode)
    if np.random.uniform() < P["gaussian_noise_probability2"]:
        out = random_add_gaussian_noise_torch(image=out, sigma_range=P["noise_range2"], clip=True, rounds=False, gray_prob=P["gray_noise_probability2"])
    else:
        out = random_add_poisson_noise_torch(image=out, scale_range=P["poisson_scale_range2"], gray_prob=P["gray_noise_probability2"], clip=True,
                                             rounds=False)
    final_size = (image_height // upscale_factor, image_width // upscale_factor)
    if np.random.uniform() < 0.5:
        # resize back -> sinc filter -> JPEG
        out = interpolate(out, size=final_size, mode=random.choice(["area", "bilinear", "bicubic"]))
        out = filter2d_torch(out, sinc_kernel)
        quality = _jpeg_quality(out, P["jpeg_range2"])
        out = jpeg_operation(torch.clamp(out, 0, 1), quality)
    else:
        # JPEG -> resize back -> sinc filter
        quality = _jpeg_quality(out, P["jpeg_range2"])
        out = jpeg_operation(torch.clamp(out, 0, 1), quality)
        out = interpolate(out, size=final_size, mode=random.choice(["area", "bilinear", "bicubic"]))
        out = filter2d_torch(out, sinc_kernel)
    lr = quantize_u8(out)
    return gt_usm, gt, lr


# ---- Real-ESRGAN's per-image filter kernels (Real_ESRGAN/dataset.py:64-133, imgproc.py:228-606) -----------------------------------
KERNEL_DELTA, KERNEL_GAUSSIAN, KERNEL_GENERALIZED, KERNEL_PLATEAU, KERNEL_SINC = 0, 1, 2, 3, 4
KERNEL_BANK_KMAX = 25
# gaussian_kernel_type name -> (kind, anisotropic); any other name takes the isotropic Gaussian, as random_mixed_kernels' else does
_MIXED_KERNEL_TYPES = {
    "isotropic": (KERNEL_GAUSSIAN, False), "anisotropic": (KERNEL_GAUSSIAN, True),
    "generalized_isotropic": (KERNEL_GENERALIZED, False), "generalized_anisotropic": (KERNEL_GENERALIZED, True),
    "plateau_isotropic": (KERNEL_PLATEAU, False), "plateau_anisotropic": (KERNEL_PLATEAU, True),
}
_KERNEL_PARAMETER_KEYS = ("sinc_kernel_size", "gaussian_kernel_range", "gaussian_kernel_type", "sinc_kernel_probability3") + tuple(
    f"{name}{n}" for n in (1, 2) for name in ("gaussian_kernel_probability", "sinc_kernel_probability", "gaussian_sigma_range",
                                              "generalized_kernel_beta_range", "plateau_kernel_beta_range"))


def _odd_kernel_size(k) -> bool:
    return isinstance(k, (int, np.integer)) and 3 <= k <= KERNEL_BANK_KMAX and k % 2 == 1


def check_realesrgan_kernel_parameters(degradation_model_parameters_dict: dict) -> None:
    """``ValueError`` unless the dict holds what ``realesrgan_kernel_draws`` and ``realesrgan_blur_kernels`` read, in a form both can use:
    every key of the reference's ``degradation_model_parameters_dict`` (realesrgan_config.py:46-65; the message names the first missing
    one), odd kernel sizes from 3 to 25 with the largest of ``gaussian_kernel_range`` last (the dataset pads to ``range[-1]``), one
    probability per kernel type, and ``lo < hi`` sigma ranges (the reference asserts that at every draw)."""
    P = degradation_model_parameters_dict
    if not isinstance(P, dict):
        raise ValueError(f"the degradation-model parameters are a dict, got {type(P).__name__}")
    for key in _KERNEL_PARAMETER_KEYS:
        if key not in P:
            raise ValueError(f"degradation-model parameters: key {key!r} is missing")
    sizes = list(P["gaussian_kernel_range"])
    if not sizes or not all(_odd_kernel_size(k) for k in sizes) or sizes[-1] != max(sizes):
        raise ValueError(f"degradation-model parameters: 'gaussian_kernel_range' holds odd sizes from 3 to {KERNEL_BANK_KMAX}, the largest last; got {sizes}")
    if not _odd_kernel_size(P["sinc_kernel_size"]):
        raise ValueError(f"degradation-model parameters: 'sinc_kernel_size' is an odd size from 3 to {KERNEL_BANK_KMAX}, got {P['sinc_kernel_size']!r}")
    types = list(P["gaussian_kernel_type"])
    for n in (1, 2):
        if not types or len(P[f"gaussian_kernel_probability{n}"]) != len(types):
            raise ValueError(f"degradation-model parameters: 'gaussian_kernel_probability{n}' holds one weight per entry of 'gaussian_kernel_type' "
                             f"({len(types)})")
        for key in (f"gaussian_sigma_range{n}", f"generalized_kernel_beta_range{n}", f"plateau_kernel_beta_range{n}"):
            if len(P[key]) != 2:
                raise ValueError(f"degradation-model parameters: {key!r} is a [lo, hi] pair, got {P[key]!r}")
        lo, hi = P[f"gaussian_sigma_range{n}"]
        if not lo < hi:
            raise ValueError(f"degradation-model parameters: 'gaussian_sigma_range{n}' needs lo < hi, got {[lo, hi]}")


def _kernel_record(kind: int, ksize: int, sigma_x=0.0, sigma_y=0.0, theta=0.0, beta=0.0, omega=0.0) -> dict:
    return {"kind": int(kind), "ksize": int(ksize), "sigma_x": float(sigma_x), "sigma_y": float(sigma_y), "theta": float(theta),
            "beta": float(beta), "omega": float(omega)}


def _draw_blur_kernel(P: dict, n: int) -> dict:
    """blur kernel ``n`` (1 or 2) of one image: dataset.py:65-86 / :92-113 with random_mixed_kernels and its _random_bivariate_* helpers"""
    sizes = P["gaussian_kernel_range"]
    ksize = random.choice(sizes)
    if np.random.uniform() < P[f"sinc_kernel_probability{n}"]:
        if ksize < int(np.median(sizes)):
            omega = np.random.uniform(np.pi / 3, np.pi)
        else:
            omega = np.random.uniform(np.pi / 5, np.pi)
        return _kernel_record(KERNEL_SINC, ksize, omega=omega)
    name = random.choices(P["gaussian_kernel_type"], P[f"gaussian_kernel_probability{n}"])[0]
    kind, anisotropic = _MIXED_KERNEL_TYPES.get(name, (KERNEL_GAUSSIAN, False))
    sigma_range = P[f"gaussian_sigma_range{n}"]
    sigma_x = np.random.uniform(sigma_range[0], sigma_range[1])
    if anisotropic:
        sigma_y = np.random.uniform(sigma_range[0], sigma_range[1])
        theta = np.random.uniform(-math.pi, math.pi)
    else:
        sigma_y, theta = sigma_x, 0.0
    beta = 0.0
    if kind != KERNEL_GAUSSIAN:
        beta_range = P[f"generalized_kernel_beta_range{n}" if kind == KERNEL_GENERALIZED else f"plateau_kernel_beta_range{n}"]
        if np.random.uniform() < 0.5:
            beta = np.random.uniform(beta_range[0], 1)
        else:
            beta = np.random.uniform(1, beta_range[1])
    return _kernel_record(kind, ksize, sigma_x, sigma_y, theta, beta)


def realesrgan_kernel_draws(batch: int, degradation_model_parameters_dict: dict) -> list:
    """Every random decision of ``DegeneratedImageDataset.__getitem__`` (Real_ESRGAN/dataset.py:64-129) and of ``random_mixed_kernels``
    with its ``_random_bivariate_*`` helpers (imgproc.py:333-576) for ``batch`` images, drawn image by image from the global ``random`` /
    ``np.random`` streams in exactly the reference's order, so that a seeded run gets the kernels the reference's loader would make.
    Per blur kernel (the first, then the second): ``random.choice(gaussian_kernel_range)``; ``np.random.uniform() <
    sinc_kernel_probabilityN``; on a hit ``np.random.uniform(pi / 3, pi)`` for a size below ``int(np.median(range))``, else
    ``uniform(pi / 5, pi)``; on a miss ``random.choices(types, probabilities)[0]``, ``uniform(sigma range)``, for the anisotropic types
    ``uniform(sigma range)`` and ``uniform(-pi, pi)``, for the generalized / plateau types ``np.random.uniform() < 0.5`` and
    ``uniform(beta0, 1)`` or ``uniform(1, beta1)``.  Then the final sinc filter: ``np.random.uniform() < sinc_kernel_probability3``; on a
    hit ``random.choice(range)`` and ``uniform(pi / 3, pi)``, on a miss the delta.  (``noise_range``: the dataset passes None and nothing
    is drawn for it.)
    One plain dict per image, ``{"kernel1", "kernel2", "sinc_kernel"}``, each a record ``{"kind", "ksize", "sigma_x", "sigma_y", "theta",
    "beta", "omega"}`` with ``kind`` 0 delta, 1 Gaussian, 2 generalized Gaussian, 3 plateau, 4 sinc -- the arguments of
    ``blur_kernel_bank``; fields a kind does not use are 0, and an isotropic kernel has ``sigma_y = sigma_x``, ``theta = 0``."""
    P = degradation_model_parameters_dict
    check_realesrgan_kernel_parameters(P)
    out = []
    for _ in range(batch):
        rec = {"kernel1": _draw_blur_kernel(P, 1), "kernel2": _draw_blur_kernel(P, 2)}
        if np.random.uniform() < P["sinc_kernel_probability3"]:
            ksize = random.choice(P["gaussian_kernel_range"])
            rec["sinc_kernel"] = _kernel_record(KERNEL_SINC, ksize, omega=np.random.uniform(np.pi / 3, np.pi))
        else:
            rec["sinc_kernel"] = _kernel_record(KERNEL_DELTA, P["sinc_kernel_size"])
        out.append(rec)
    return out


def blur_kernel_bank(kind, ksize, params, kmax: int, device=None) -> Tensor:
    """srganfd_blur_kernel_bank: ``n`` filter kernels from their parameters in one launch, ``(n, kmax, kmax)`` fp32 on the GPU.  ``kind``
    (n integers: 0 delta, 1 Gaussian, 2 generalized Gaussian, 3 plateau, 4 sinc), ``ksize`` (n odd sizes from 3 to ``kmax`` <= 25; kernel
    i sits centred in its array with exact zeros around it; ignored by a delta) and ``params`` ((n, 5) floats: sigma_x, sigma_y, theta,
    beta, omega) are host arrays or lists, uploaded with one small copy each.  fp64 arithmetic, one rounding to fp32 (include/srganfd.h
    has the formulas); the launch goes to the current stream of ``device`` (default: the current GPU)."""
    kd, ks = np.asarray(kind), np.asarray(ksize)
    if kd.ndim != 1 or kd.size == 0 or kd.dtype.kind not in "iu" or ks.dtype.kind not in "iu" or ks.shape != kd.shape:
        raise A.SrganfdError(f"blur_kernel_bank: kind and ksize hold one integer per kernel (at least one), got {kd.dtype} {kd.shape} and {ks.dtype} {ks.shape}")
    try:
        pr = np.ascontiguousarray(np.asarray(params), dtype=np.float64)
    except (TypeError, ValueError):
        raise A.SrganfdError("blur_kernel_bank: params holds 5 numbers per kernel (sigma_x, sigma_y, theta, beta, omega)") from None
    if pr.shape != (kd.size, 5):
        raise A.SrganfdError(f"blur_kernel_bank: params is (n, 5) = ({kd.size}, 5): sigma_x, sigma_y, theta, beta, omega; got {pr.shape}")
    if not isinstance(kmax, (int, np.integer)):
        raise A.SrganfdError(f"blur_kernel_bank: kmax is an odd integer from 3 to {KERNEL_BANK_KMAX}, got {kmax!r}")
    kd, ks = np.ascontiguousarray(kd, dtype=np.int32), np.ascontiguousarray(ks, dtype=np.int32)
    host = [torch.from_numpy(a) for a in (kd, ks, pr)]
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        _need_gpu(host[0], "blur_kernel_bank")
    with torch.cuda.device(dev):
        kd_dev, ks_dev, pr_dev = (t.to(dev) for t in host)
        out = torch.empty(kd.size, int(kmax), int(kmax), dtype=torch.float32, device=dev)
        A.check(A.lib().srganfd_blur_kernel_bank(kd_dev.data_ptr(), ks_dev.data_ptr(), pr_dev.data_ptr(), kd.ctypes.data, ks.ctypes.data, kd.size,
                                                 int(kmax), out.data_ptr(), A.stream_ptr()), "blur_kernel_bank")
    return out


_KERNEL_PARAM_FIELDS = ("sigma_x", "sigma_y", "theta", "beta", "omega")


def realesrgan_blur_kernels(draws: list, degradation_model_parameters_dict: dict, device=None):
    """The three filter kernels of every image of ``draws`` (``realesrgan_kernel_draws``) as the reference's collated batch holds them
    (Real_ESRGAN/dataset.py:72-133): ``(gaussian_kernel1, gaussian_kernel2, sinc_kernel)``, each (B, K, K) fp32 on the GPU with
    K = ``gaussian_kernel_range[-1]`` for the first two and ``sinc_kernel_size`` for the third, every kernel centred in its array -- what
    ``degradation_process`` / ``filter2d_torch`` take.  One ``blur_kernel_bank`` launch for all 3 B kernels when the two sizes agree (the
    reference's configs: 21), else two.  ``ValueError`` for a drawn sinc filter larger than ``sinc_kernel_size`` (the reference would hand
    its collate function tensors of different shapes)."""
    P = degradation_model_parameters_dict
    check_realesrgan_kernel_parameters(P)
    b = len(draws)
    if b == 0:
        raise ValueError("realesrgan_blur_kernels: no draws")
    k_blur, k_sinc = int(P["gaussian_kernel_range"][-1]), int(P["sinc_kernel_size"])
    recs = [rec[name] for name in ("kernel1", "kernel2", "sinc_kernel") for rec in draws]          # (3, B) order: each output is one slice
    for n, r in enumerate(recs[2 * b:]):
        if r["kind"] != KERNEL_DELTA and r["ksize"] > k_sinc:
            raise ValueError(f"realesrgan_blur_kernels: image {n} drew a {r['ksize']} x {r['ksize']} sinc filter, larger than sinc_kernel_size = {k_sinc}")
    kind = np.array([r["kind"] for r in recs], dtype=np.int32)
    ksize = np.array([r["ksize"] for r in recs], dtype=np.int32)
    params = np.array([[r[f] for f in _KERNEL_PARAM_FIELDS] for r in recs], dtype=np.float64)
    if k_blur == k_sinc:
        bank = blur_kernel_bank(kind, ksize, params, k_blur, device)
        return bank[:b], bank[b:2 * b], bank[2 * b:]
    blur = blur_kernel_bank(kind[:2 * b], ksize[:2 * b], params[:2 * b], k_blur, device)
    return blur[:b], blur[b:], blur_kernel_bank(kind[2 * b:], ksize[2 * b:], params[2 * b:], k_sinc, device)


# ---- BSRGAN / A-ESRGAN blind degradation (BSRGAN/imgproc.py:161-225, 284-293, 492-562; the same text in A-ESRGAN/imgproc.py) ------
def jpeg_compression(image: Tensor, quality) -> Tensor:
    """imgproc._add_jpeg_compression (BSRGAN/imgproc.py:284-293) for a batch, at given qualities: ``uint8(round(clip(x, 0, 1) * 255))``,
    a real baseline JPEG encode and decode (what ``cv2.imencode`` / ``cv2.imdecode`` run through libjpeg: 4:2:0, integer DCT, fancy
    upsampling -- srganfd_jpeg_roundtrip computes the library's bytes), ``float32(u8) / 255``.  ``image``: (B, 3, H, W) or (3, H, W) RGB
    on the GPU; ``quality``: an int, a sequence or an integer tensor with one entry per image, 1..100, where 0 returns that image
    unchanged bit for bit (a ``jpeg_prob`` miss inside a batch).  Values that live on the host are validated; an integer tensor already
    on the GPU is used as it is (no synchronisation; the kernel clamps 1..100).  Not differentiable: ``DiffJPEG`` is the other one."""
    if not torch.is_tensor(image) or image.dim() not in (3, 4):
        raise A.SrganfdError("jpeg_compression takes (3, H, W) or (B, 3, H, W) tensors")
    _need_gpu(image, "jpeg_compression")
    x = image.detach().contiguous().float()
    x4 = x if x.dim() == 4 else x.unsqueeze(0)
    b, c, h, w = x4.shape
    q_host = None
    if torch.is_tensor(quality) and quality.is_cuda:
        if quality.dtype not in (torch.int32, torch.int64) or quality.numel() != b:
            raise A.SrganfdError("jpeg_compression: a quality tensor holds one integer per image")
        q_dev = quality.to(torch.int32).contiguous()
    else:
        q_host = _per_image_int(quality, b, "jpeg_compression: quality")
        q_dev = torch.from_numpy(q_host).to(x.device)
    return _jpeg_roundtrip(x4, q_dev, q_host).view(x.shape)


def _per_image_int(v, b: int, what: str) -> np.ndarray:
    if isinstance(v, (int, np.integer)):
        return np.full(b, int(v), dtype=np.int32)
    a = np.asarray(v.cpu() if torch.is_tensor(v) else v)
    if a.dtype.kind not in "iu" or a.size != b:
        raise A.SrganfdError(f"{what} holds one integer per image ({b}), got {a.dtype} x {a.size}")
    return np.ascontiguousarray(a.reshape(b), dtype=np.int32)


def _jpeg_roundtrip(x: Tensor, q_dev: Tensor, q_host) -> Tensor:
    b, c, h, w = x.shape
    L = A.lib()
    nbytes = L.srganfd_jpeg_workspace_bytes(b, h, w)
    ws = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=x.device)
    out = torch.empty_like(x)
    A.check(L.srganfd_jpeg_roundtrip(x.data_ptr(), b, c, h, w, q_dev.data_ptr(), q_host.ctypes.data if q_host is not None else None, ws.data_ptr(),
                                     out.data_ptr(), A.stream_ptr()), "jpeg_roundtrip")
    return out


def _filter2d_mirror_f64(x: Tensor, kernels: Tensor, ksize_dev: Tensor, ksize_host: np.ndarray) -> Tensor:
    """srganfd_filter2d_mirror_f64: image n of ``x`` with its own ``ksize[n]``-sized kernel (0: copied through), centred in ``kernels[n]``"""
    b, c, h, w = x.shape
    out = torch.empty_like(x)
    A.check(A.lib().srganfd_filter2d_mirror_f64(x.data_ptr(), kernels.data_ptr(), kernels.shape[-1], ksize_dev.data_ptr(), ksize_host.ctypes.data,
                                                b, c, h, w, out.data_ptr(), A.stream_ptr()), "filter2d_mirror_f64")
    return out


def filter2d_mirror_f64(image: Tensor, kernels, ksize) -> Tensor:
    """``ndimage.convolve(image, k[:, :, None], mode='mirror')`` (BSRGAN/imgproc.py:223) for a batch whose images each have a kernel of
    their own: ``image`` (B, C, H, W) on the GPU, ``kernels`` (B, kmax, kmax) float64 (array or tensor) with image n's ``ksize[n]``-sized
    kernel centred in its array, ``ksize`` B odd sizes from 3 to kmax <= 25 or 0 (that image is returned unchanged).  fp64 multiply-adds,
    one rounding to float32: scipy's values.  Cross-correlation, which for point-symmetric kernels is scipy's convolution."""
    if not torch.is_tensor(image) or image.dim() != 4:
        raise A.SrganfdError("filter2d_mirror_f64 takes a (B, C, H, W) tensor")
    _need_gpu(image, "filter2d_mirror_f64")
    x = image.detach().contiguous().float()
    ks = _per_image_int(ksize, x.shape[0], "filter2d_mirror_f64: ksize")
    kk = torch.as_tensor(kernels).to(device=x.device, dtype=torch.float64).contiguous()
    if kk.dim() != 3 or kk.shape[0] != x.shape[0] or kk.shape[1] != kk.shape[2]:
        raise A.SrganfdError(f"filter2d_mirror_f64: kernels are (B, kmax, kmax), got {tuple(kk.shape)} for {x.shape[0]} images")
    return _filter2d_mirror_f64(x, kk, torch.from_numpy(ks).to(x.device), ks)


BSRGAN_KMAX = 25             # _add_blur draws 2 * randint(2, 11) + 3: 7 .. 25
_CV2_INTERP = {1: "bilinear", 2: "bicubic", 3: "area"}      # cv2.INTER_LINEAR / INTER_CUBIC / INTER_AREA


def _fspecial_gaussian(hsize: int, sigma: float) -> np.ndarray:
    """imgproc._fspecial_gaussian (BSRGAN/imgproc.py:161-172; ``np.finfo`` for the ``scipy.finfo`` that scipy no longer has)"""
    half = (hsize - 1.0) / 2.0
    x, y = np.meshgrid(np.arange(-half, half + 1), np.arange(-half, half + 1))
    h = np.exp(-(x * x + y * y) / (2 * sigma * sigma))
    h[h < np.finfo(float).eps * h.max()] = 0
    sumh = h.sum()
    if sumh != 0:
        h = h / sumh
    return h


def _gm_blur_kernel(cov: np.ndarray, size: int) -> np.ndarray:
    """imgproc._gm_blur_kernel (:186-197) at mean 0: the bivariate normal density on the centred grid, normalised to sum 1.  The density is
    written out (scipy is not a dependency): exp(-x' inv(cov) x / 2) / (2 pi sqrt(det cov))"""
    c = np.arange(size) - size / 2.0 - 0.5 + 1
    cx, cy = np.meshgrid(c, c)                                # k[y, x] = pdf([cx, cy])
    cov = (cov + cov.T) / 2
    inv = np.linalg.inv(cov)
    maha = inv[0, 0] * cx * cx + (inv[0, 1] + inv[1, 0]) * cx * cy + inv[1, 1] * cy * cy
    k = np.exp(-0.5 * maha) / (2 * np.pi * np.sqrt(np.linalg.det(cov)))
    return k / np.sum(k)


def _anisotropic_gaussian(ksize: int, theta: float, l1: float, l2: float) -> np.ndarray:
    """imgproc._anisotropic_gaussian (:201-208)"""
    v = np.dot(np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]]), np.array([1., 0.]))
    V = np.array([[v[0], v[1]], [v[1], -v[0]]])
    D = np.array([[l1, 0], [0, l2]])
    return _gm_blur_kernel(np.dot(np.dot(V, D), np.linalg.inv(V)), ksize)


def bsrgan_degradation_draws(batch: int, upscale_factor: int, jpeg_prob: float = 0.9, scale2_prob: float = 0.25) -> list:
    """Every random decision of ``degradation_process`` (BSRGAN/imgproc.py:492-562) for ``batch`` images, drawn image by image from the
    global ``random`` and ``np.random`` streams in exactly the reference's order, so that a seeded run degrades as the reference's loader
    would: [factor 4 only: ``random.random() < scale2_prob``; if so ``np.random.rand() < 0.5`` and, for the cv2 branch,
    ``random.choice([1, 2, 3])``], ``random.sample(range(6), 6)``, then per live op in the shuffled order -- a blur: ``random.random() <
    0.5``, then ``l1``, ``l2``, ``randint(2, 11)``, ``random.random() * pi`` (anisotropic) or ``randint(2, 11)``, ``wd * random.random()``
    (isotropic); the JPEG: ``random.random() < jpeg_prob`` and ``randint(30, 95)`` on a hit -- and the final ``randint(30, 95)``.  Ops 2,
    3 and 4 (the two resizes and the noise) begin with ``continue`` in the reference and draw nothing.
    One plain dict per image: ``upscale_factor`` (as passed), ``half`` (None, "imresize" or "cv2"), ``interp`` (cv2's code 1 / 2 / 3 =
    bilinear / bicubic / area, or None), ``sf`` (2 after a half-step), ``order`` (the shuffle), ``ops`` (the live ops in order:
    ``("blur", {"kind": "aniso", "ksize", "theta", "l1", "l2"})``, ``("blur", {"kind": "iso", "ksize", "sigma"})``, ``("jpeg", quality or
    0 on a miss)``) and ``final_quality``."""
    out = []
    for _ in range(batch):
        rec = {"upscale_factor": upscale_factor, "half": None, "interp": None, "sf": upscale_factor}
        if upscale_factor == 4 and random.random() < scale2_prob:
            if np.random.rand() < 0.5:
                rec["half"], rec["interp"] = "cv2", random.choice([1, 2, 3])
            else:
                rec["half"] = "imresize"
            rec["sf"] = 2
        order = random.sample(range(6), 6)
        idx1, idx2 = order.index(2), order.index(3)
        if idx1 > idx2:
            order[idx1], order[idx2] = order[idx2], order[idx1]
        rec["order"] = order
        wd, wd2 = 2.0 + 0.2 * rec["sf"], 4.0 + rec["sf"]
        ops = []
        for i in order:
            if i in (0, 1):
                if random.random() < 0.5:
                    l1 = wd2 * random.random()
                    l2 = wd2 * random.random()
                    ksize = 2 * random.randint(2, 11) + 3
                    ops.append(("blur", {"kind": "aniso", "ksize": ksize, "theta": random.random() * np.pi, "l1": l1, "l2": l2}))
                else:
                    ksize = 2 * random.randint(2, 11) + 3
                    ops.append(("blur", {"kind": "iso", "ksize": ksize, "sigma": wd * random.random()}))
            elif i == 5:
                ops.append(("jpeg", random.randint(30, 95) if random.random() < jpeg_prob else 0))
        rec["ops"] = ops
        rec["final_quality"] = random.randint(30, 95)
        out.append(rec)
    return out


def bsrgan_blur_kernels(draws: list, upscale_factor: int):
    """The two blur kernels of every image of ``draws`` (``_add_blur``, BSRGAN/imgproc.py:212-225), on the host in float64: ``(kernels
    (B, 2, 25, 25)`` with each k x k kernel centred in its 25 x 25 array and zeros around it, ``ksize (B, 2) int32)``, the blurs in the
    order the image runs them.  ``upscale_factor`` is the one the draws were made for (the widths ``wd``, ``wd2`` of an image that took the
    half-step come from its updated factor and are already in its draws)."""
    kernels = np.zeros((len(draws), 2, BSRGAN_KMAX, BSRGAN_KMAX), dtype=np.float64)
    ksize = np.zeros((len(draws), 2), dtype=np.int32)
    for n, rec in enumerate(draws):
        if rec["upscale_factor"] != upscale_factor:
            raise ValueError(f"bsrgan_blur_kernels: image {n} was drawn for factor {rec['upscale_factor']}, not {upscale_factor}")
        blurs = [p for kind, p in rec["ops"] if kind == "blur"]
        for j, p in enumerate(blurs):
            k = _anisotropic_gaussian(p["ksize"], p["theta"], p["l1"], p["l2"]) if p["kind"] == "aniso" else _fspecial_gaussian(p["ksize"], p["sigma"])
            o = (BSRGAN_KMAX - p["ksize"]) // 2
            kernels[n, j, o:o + p["ksize"], o:o + p["ksize"]] = k
            ksize[n, j] = p["ksize"]
    return kernels, ksize


def _bsrgan_programs(draws: list, kernels: np.ndarray, ksize: np.ndarray, idx: list):
    """the images ``idx`` as three rounds of (blur | JPEG): per round the kernel array, the blur sizes (0: no blur this round) and the
    JPEG qualities (0: none), plus the final qualities"""
    n = len(idx)
    kr = np.zeros((3, n, BSRGAN_KMAX, BSRGAN_KMAX), dtype=np.float64)
    ks = np.zeros((3, n), dtype=np.int32)
    qs = np.zeros((4, n), dtype=np.int32)
    for j, i in enumerate(idx):
        nb = 0
        for r, (kind, p) in enumerate(draws[i]["ops"]):
            if kind == "blur":
                kr[r, j], ks[r, j] = kernels[i, nb], ksize[i, nb]
                nb += 1
            else:
                qs[r, j] = p
        qs[3, j] = draws[i]["final_quality"]
    return kr, ks, qs


def degradation_process_bsrgan(gt: Tensor, upscale_factor: int, jpeg_prob: float = 0.9, scale2_prob: float = 0.25, draws: list = None) -> Tensor:
    """imgproc.degradation_process (BSRGAN/imgproc.py:492-562, dataset.py:83; A-ESRGAN's is the same text) for a whole GT batch on the GPU:
    per image an optional half-size step (factor 4 only), two Gaussian blurs and an optional JPEG round trip in a shuffled order, a final
    JPEG round trip and ``image_resize(1 / factor)``.  ``gt``: (B, 3, H, W) fp32 RGB in [0, 1]; returns (B, 3, H / factor, W / factor).
    ``draws``: the per-image records of ``bsrgan_degradation_draws``; None draws them here, consuming the global ``random`` /
    ``np.random`` streams exactly as the reference does image by image.
    Images that took the half-step form a second sub-batch at (H / 2, W / 2) that runs with factor 2.  Each image's program is at most
    three ops, run in three rounds; a round is one batched blur launch (srganfd_filter2d_mirror_f64, sizes 0 copy through) and one
    batched JPEG launch (srganfd_jpeg_roundtrip, quality 0 copies through) per sub-batch, so nothing is gathered per image.  The blur
    accumulates in fp64 like scipy's and the JPEG is the library's integer pipeline, so everything before the last ``image_resize`` lands on
    the reference's float32 values.  The reference's ops 2, 3, 4 are dead code (they begin with ``continue``) and are not here.
    ``ValueError``: a factor below 1, sizes the factor does not divide (odd sizes at factor 4 included), images whose shorter side -- after
    the possible half-step -- is 12 or less (a 25-tap mirror does not fit), draws that do not match the batch."""
    if not torch.is_tensor(gt) or gt.dim() != 4 or gt.shape[1] != 3:
        raise A.SrganfdError("degradation_process_bsrgan takes a (B, 3, H, W) tensor")
    b, _, h, w = gt.shape
    if not (isinstance(upscale_factor, int) and upscale_factor >= 1):
        raise ValueError(f"degradation_process_bsrgan: upscale_factor must be a positive integer, got {upscale_factor}")
    if upscale_factor == 4 and (h % 2 or w % 2):
        raise ValueError(f"degradation_process_bsrgan: {h} x {w} is odd; factor 4 may halve the image first")
    if h % upscale_factor or w % upscale_factor:
        raise ValueError(f"degradation_process_bsrgan: {h} x {w} is not divisible by the factor {upscale_factor}")
    if (min(h, w) / 2 if upscale_factor == 4 else min(h, w)) <= BSRGAN_KMAX // 2:
        raise ValueError(f"degradation_process_bsrgan: {h} x {w} is too small at factor {upscale_factor}: the 25-tap blur mirrors 12 samples "
                         "of the image (of its half-size copy at factor 4)")
    if draws is not None and (len(draws) != b or any(r["upscale_factor"] != upscale_factor for r in draws)):
        raise ValueError(f"degradation_process_bsrgan: draws are for {len(draws)} images"
                         f" at factor {sorted(set(r['upscale_factor'] for r in draws))}, the batch is {b} at factor {upscale_factor}")
    _need_gpu(gt, "degradation_process_bsrgan")
    if draws is None:
        draws = bsrgan_degradation_draws(b, upscale_factor, jpeg_prob, scale2_prob)
    kernels, ksize = bsrgan_blur_kernels(draws, upscale_factor)
    x = gt.detach().contiguous().float()
    dev = x.device
    out = torch.empty(b, 3, h // upscale_factor, w // upscale_factor, dtype=torch.float32, device=dev)
    full = [i for i, r in enumerate(draws) if r["half"] is None]
    half = [i for i, r in enumerate(draws) if r["half"] is not None]
    batches = []
    if full:
        batches.append((full, x if len(full) == b else x[torch.as_tensor(full, device=dev)], upscale_factor))
    if half:
        xh = torch.empty(len(half), 3, h // 2, w // 2, dtype=torch.float32, device=dev)
        groups = {}
        for j, i in enumerate(half):
            groups.setdefault(draws[i]["interp"], []).append((j, i))
        for interp, members in groups.items():
            src = x[torch.as_tensor([i for _, i in members], device=dev)]
            y = image_resize(src, 1 / 2, True) if interp is None else interpolate(src, scale_factor=0.5, mode=_CV2_INTERP[interp])
            xh[torch.as_tensor([j for j, _ in members], device=dev)] = torch.clamp(y, 0.0, 1.0)
        batches.append((half, xh, 2))
    for idx, y, sf in batches:
        kr, ks, qs = _bsrgan_programs(draws, kernels, ksize, idx)
        ks_dev, qs_dev = torch.from_numpy(ks).to(dev), torch.from_numpy(qs).to(dev)
        kr_dev = torch.from_numpy(kr).to(dev) if ks.any() else None
        for r in range(3):
            if ks[r].any():
                y = _filter2d_mirror_f64(y, kr_dev[r], ks_dev[r], ks[r])
            if qs[r].any():
                y = _jpeg_roundtrip(y, qs_dev[r], qs[r])
        y = _jpeg_roundtrip(y, qs_dev[3], qs[3])
        y = image_resize(y, 1 / sf)
        if len(idx) == b:
            return y
        out[torch.as_tensor(idx, device=dev)] = y
    return out


# ---- batch augmentation of the Real-ESRGAN loop (train_realesrgan.py:400-404) ------------------------------------------------
def _as_list(v):
    return (v, True) if isinstance(v, list) else ([v], False)


def _crop_rot_flip(t: Tensor, top: int, left: int, ph: int, pw: int, op: int) -> Tensor:
    _need_gpu(t, "augmentation")
    x = t.detach().contiguous().float()
    b, c, h, w = x.shape
    out = torch.empty(b, c, ph, pw, dtype=torch.float32, device=x.device)
    A.check(A.lib().srganfd_crop_rot_flip(x.data_ptr(), out.data_ptr(), b * c, h, w, top, left, ph, pw, op, A.stream_ptr()), "crop_rot_flip")
    return out.to(t.dtype)


def random_crop_torch(gt_images, lr_images, gt_patch_size: int, upscale_factor: int):
    """imgproc.random_crop_torch (Real_ESRGAN/imgproc.py:2081-2155), tensor inputs: one LR window drawn with ``random.randint``
    (row, then column) for every tensor of both lists, the GT window at upscale_factor times its origin."""
    gts, _ = _as_list(gt_images)
    lrs, _ = _as_list(lr_images)
    lh, lw = lrs[0].size()[-2:]
    lps = gt_patch_size // upscale_factor
    lr_top = random.randint(0, lh - lps)
    lr_left = random.randint(0, lw - lps)
    lrs = [_crop_rot_flip(t, lr_top, lr_left, lps, lps, 0) for t in lrs]
    gts = [_crop_rot_flip(t, int(lr_top * upscale_factor), int(lr_left * upscale_factor), gt_patch_size, gt_patch_size, 0) for t in gts]
    return (gts[0] if len(gts) == 1 else gts), (lrs[0] if len(lrs) == 1 else lrs)


def random_rotate_torch(gt_images, lr_images, upscale_factor: int, angles: list, gt_center=None, lr_center=None, rotate_scale_factor: float = 1.0):
    """imgproc.random_rotate_torch (Real_ESRGAN/imgproc.py:2158-2230), tensor inputs: one angle drawn with ``random.choice``;
    the reference rotates with torchvision about the default centre [w // 2, h // 2], which for the multiples of 90 degrees the
    train loops pass (train_realesrgan.py:401) and square even-sized batches is an exact counter-clockwise quarter-turn
    permutation -- the only case with a HIP path."""
    angle = random.choice(angles)
    gts, _ = _as_list(gt_images)
    lrs, _ = _as_list(lr_images)
    if gt_center is not None or lr_center is not None or rotate_scale_factor != 1.0 or angle % 90 != 0:
        raise A.SrganfdError("random_rotate_torch: only default-centre rotations by multiples of 90 degrees have a HIP path")
    op = (angle // 90) % 4
    out = []
    for group in (gts, lrs):
        res = []
        for t in group:
            h, w = t.shape[-2:]
            if op in (1, 3) and (h != w or h % 2):
                raise A.SrganfdError("random_rotate_torch: quarter turns need square, even-sized images")
            res.append(_crop_rot_flip(t, 0, 0, h, w, op))
        out.append(res)
    return (out[0][0] if len(out[0]) == 1 else out[0]), (out[1][0] if len(out[1]) == 1 else out[1])


def _random_flip(gt_images, lr_images, p: float, op: int):
    flip_prob = random.random()
    gts, _ = _as_list(gt_images)
    lrs, _ = _as_list(lr_images)
    if flip_prob > p:
        lrs = [_crop_rot_flip(t, 0, 0, t.shape[-2], t.shape[-1], op) for t in lrs]
        gts = [_crop_rot_flip(t, 0, 0, t.shape[-2], t.shape[-1], op) for t in gts]
    return (gts[0] if len(gts) == 1 else gts), (lrs[0] if len(lrs) == 1 else lrs)


def random_horizontally_flip_torch(gt_images, lr_images, p: float = 0.5):
    """imgproc.random_horizontally_flip_torch (Real_ESRGAN/imgproc.py:2233-2275): flips when ``random.random() > p``"""
    return _random_flip(gt_images, lr_images, p, 4)


def random_vertically_flip_torch(gt_images, lr_images, p: float = 0.5):
    """imgproc.random_vertically_flip_torch (Real_ESRGAN/imgproc.py:2278-2320)"""
    return _random_flip(gt_images, lr_images, p, 5)
