"""PSNR, SSIM and NIQE of the validation loop (reference: BSRGAN/image_quality_assessment.py:361-418, :420-532 and
:1138-1333, used at train_bsrgan.py:545-590), and LPIPS (the `lpips` package's ``LPIPS(net='alex')`` of train_bsrgan.py:115,571;
sr_gan_fd_amd/lpips.py), re-exported here so that one import binds all four validation metrics."""
from __future__ import annotations

import numpy as np
import torch
from torch import Tensor, nn

from . import _abi as A
from .lpips import LPIPS  # noqa: F401


class PSNR(nn.Module):
    """Same constructor and call as the reference's ``PSNR(crop_border, only_test_y_channel)``: inputs (N,C,H,W) RGB in
    [0,1]; returns the per-image PSNR in dB as a float64 tensor of shape (N,).  One fused HIP pass (border crop, BT.601
    luma, fp64 squared-error reduction) instead of the reference's slice / matmul / cast / mean chain."""

    def __init__(self, crop_border: int, only_test_y_channel: bool) -> None:
        super().__init__()
        self.crop_border = crop_border
        self.only_test_y_channel = only_test_y_channel

    def forward(self, raw_tensor: Tensor, dst_tensor: Tensor) -> Tensor:
        assert raw_tensor.shape == dst_tensor.shape, \
            f"Supplied images have different sizes {str(raw_tensor.shape)} and {str(dst_tensor.shape)}"
        if not raw_tensor.is_cuda:
            raise A.SrganfdError("PSNR: tensors must be on the GPU (the HIP library is the product; no CPU fallback)")
        a, b = raw_tensor.detach().contiguous().float(), dst_tensor.detach().contiguous().float()
        n, c, h, w = a.shape
        out = torch.empty(n, dtype=torch.float64, device=a.device)
        ws = torch.empty(n * 64, dtype=torch.float64, device=a.device)
        A.check(A.lib().srganfd_psnr(a.data_ptr(), b.data_ptr(), n, c, h, w, self.crop_border, 1 if self.only_test_y_channel else 0,
                                     out.data_ptr(), ws.data_ptr(), A.stream_ptr()), "psnr")
        return out


def gaussian_kernel_1d(window_size: int, sigma: float) -> np.ndarray:
    """The filter the reference obtains from ``cv2.getGaussianKernel(window_size, sigma)`` (OpenCV is not a dependency
    here): OpenCV's documented formula G_i = alpha * exp(-(i - (ksize-1)/2)^2 / (2 sigma^2)) with sum(G) = 1, and
    sigma = 0.3*((ksize-1)*0.5 - 1) + 0.8 when a non-positive sigma is passed.  fp64 column vector (ksize, 1)."""
    if sigma <= 0:
        sigma = 0.3 * ((window_size - 1) * 0.5 - 1) + 0.8
    x = np.arange(window_size, dtype=np.float64) - (window_size - 1) * 0.5
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return (g / g.sum()).reshape(window_size, 1)


class SSIM(nn.Module):
    """Same constructor (including the reference's ``only_only_test_y_channel`` spelling) and call as the reference's
    ``SSIM`` (image_quality_assessment.py:497-532): inputs (N,C,H,W) RGB in [0,1]; returns the per-image SSIM as a float32
    tensor of shape (N,).  One fused HIP pass per image tile (crop, BT.601 luma, the five fp64 window moments, the SSIM
    map and its mean) instead of five grouped conv2d calls over fp64 copies."""

    def __init__(self, crop_border: int, only_only_test_y_channel: bool, window_size: int = 11, gaussian_sigma: float = 1.5) -> None:
        super().__init__()
        self.crop_border = crop_border
        self.only_test_y_channel = only_only_test_y_channel
        self.window_size = window_size
        g = gaussian_kernel_1d(window_size, gaussian_sigma)
        self.gaussian_kernel_window = np.outer(g, g.transpose())
        self._window_dev = None

    def forward(self, raw_tensor: Tensor, dst_tensor: Tensor) -> Tensor:
        assert raw_tensor.shape == dst_tensor.shape, \
            f"Supplied images have different sizes {str(raw_tensor.shape)} and {str(dst_tensor.shape)}"
        if not raw_tensor.is_cuda:
            raise A.SrganfdError("SSIM: tensors must be on the GPU (the HIP library is the product; no CPU fallback)")
        a, b = raw_tensor.detach().contiguous().float(), dst_tensor.detach().contiguous().float()
        n, c, h, w = a.shape
        if self._window_dev is None or self._window_dev.device != a.device:
            self._window_dev = torch.from_numpy(np.ascontiguousarray(self.gaussian_kernel_window, dtype=np.float64)).to(a.device)
        y = 1 if self.only_test_y_channel else 0
        L = A.lib()
        nws = L.srganfd_ssim_workspace_doubles(n, c, h, w, self.crop_border, y, self.window_size)
        out = torch.empty(n, dtype=torch.float32, device=a.device)
        ws = torch.empty(max(int(nws), 1), dtype=torch.float64, device=a.device)
        A.check(L.srganfd_ssim(a.data_ptr(), b.data_ptr(), n, c, h, w, self.crop_border, y, self._window_dev.data_ptr(), self.window_size,
                               out.data_ptr(), ws.data_ptr(), A.stream_ptr()), "ssim")
        return out


NIQE_FEATURES = 36


def niqe_tables() -> Tensor:
    """(4, 9801) fp64, built once per NIQE module: the reference's AGGD shape grid (``torch.arange(0.2, 10.001, 0.001)``, float32,
    widened), its ``r_gam`` (image_quality_assessment.py:1156-1157) and the two gamma-function factors of the features
    (:1175-1178, :1209), all from ``torch.lgamma`` in fp64 on the host as the reference computes them on every call."""
    aggd = torch.arange(0.2, 10 + 0.001, 0.001).to(torch.float64)
    l1, l2, l3 = torch.lgamma(1. / aggd), torch.lgamma(2. / aggd), torch.lgamma(3. / aggd)
    r_gam = (2 * l2 - (l1 + l3)).exp()
    if not bool((r_gam[1:] > r_gam[:-1]).all()):
        raise A.SrganfdError("NIQE: the r_gam table does not rise strictly; the kernel's bisection needs that")
    return torch.stack([aggd, r_gam, (l1 - l3).exp().sqrt(), (l2 - l1).exp()]).contiguous()


class NIQE(nn.Module):
    """Same constructor and call as the reference's ``NIQE(crop_border, niqe_model_path, block_size_height, block_size_width)``
    (image_quality_assessment.py:1290-1333): input (N,3,H,W) RGB in [0,1] on the GPU; returns the per-image NIQE score as a float64
    tensor of shape (N,) (the reference squeezes N = 1 to a 0-dim tensor; ``.item()`` works on both).

    The model file (``mu_prisparam``, ``cov_prisparam``) is read once, here, with ``scipy.io.loadmat``; the reference reads it on
    every call.  Luma, the MSCN maps at both scales, the block statistics, the AGGD fits and the half-size resize are four HIP
    launches (csrc/iqa.hip) writing an (N, blocks, 36) fp64 feature matrix; the reference's float32 resize is reproduced, the scores
    depend on it.  The last step, 36 x 36 per image (nanmean / nancov over blocks, pseudo-inverse, quadratic form), is a handful of
    fp64 torch ops on the device and takes most of the time (DESIGN.md 4a has the numbers).  Host synchronisation: the HIP launches
    and this module read nothing back, but ``torch.linalg.pinv`` checks its solver's status on the host, so ``forward`` does
    synchronise once, inside that call.  Blocks whose features hold a NaN are left out of the covariance per image (the
    reference's reshape assumes that every image of the batch loses the same number of blocks)."""

    def __init__(self, crop_border: int, niqe_model_path: str, block_size_height: int = 96, block_size_width: int = 96) -> None:
        super().__init__()
        self.crop_border = crop_border
        self.niqe_model_path = niqe_model_path
        self.block_size_height = block_size_height
        self.block_size_width = block_size_width
        from scipy.io import loadmat          # here, not at module import: the package imports without scipy
        try:
            model = loadmat(niqe_model_path)
        except (OSError, ValueError) as e:
            raise A.SrganfdError(f"NIQE: cannot read the model file {niqe_model_path!r}: {e}") from e
        for key in ("mu_prisparam", "cov_prisparam"):
            if key not in model:
                raise A.SrganfdError(f"NIQE: the model file {niqe_model_path!r} has no '{key}'")
        # through float32 like the reference's .to(tensor) with a float32 image, then fp64 for the arithmetic
        self.mu_pris_param = torch.from_numpy(np.ravel(model["mu_prisparam"]).astype(np.float32)).to(torch.float64)
        self.cov_pris_param = torch.from_numpy(np.asarray(model["cov_prisparam"]).astype(np.float32)).to(torch.float64)
        if self.mu_pris_param.shape != (NIQE_FEATURES,) or self.cov_pris_param.shape != (NIQE_FEATURES, NIQE_FEATURES):
            raise A.SrganfdError(f"NIQE: the model file {niqe_model_path!r} holds mu_prisparam {tuple(model['mu_prisparam'].shape)} and "
                                 f"cov_prisparam {tuple(model['cov_prisparam'].shape)}; 36 and 36 x 36 are needed")
        # a symmetric model covariance (the usual case) lets the pseudo-inverse go through the symmetric eigensolver, ten times
        # quicker on the device than the general SVD; the sum with the blocks' covariance is symmetric up to rounding either way
        self._symmetric = bool(torch.equal(self.cov_pris_param, self.cov_pris_param.T))
        self._tables = niqe_tables()
        self._dev = None

    def _on(self, device):
        if self._dev is None or self._dev[0] != device:
            self._dev = (device, self._tables.to(device), self.mu_pris_param.to(device), self.cov_pris_param.to(device))
        return self._dev[1:]

    def features(self, raw_tensor: Tensor):
        """(features (N, blocks, 36), luma plane (N, lh, lw), half-size plane (N, lh/2, lw/2) in [0,1]), all fp64 on the device"""
        if not raw_tensor.is_cuda:
            raise A.SrganfdError("NIQE: the tensor must be on the GPU (the HIP library is the product; no CPU fallback)")
        a = raw_tensor.detach().contiguous().float()
        if a.dim() != 4:
            raise A.SrganfdError(f"NIQE: needs an (N,3,H,W) tensor, got shape {tuple(a.shape)}")
        n, c, h, w = a.shape
        bh, bw = self.block_size_height, self.block_size_width
        L = A.lib()
        nws = int(L.srganfd_niqe_workspace_doubles(n, c, h, w, self.crop_border, bh, bw))
        if nws < 0:
            A.check(-1, "niqe")
        table = self._on(a.device)[0]
        lh, lw = (h - 2 * self.crop_border) // bh * bh, (w - 2 * self.crop_border) // bw * bw
        feat = torch.empty(n, (lh // bh) * (lw // bw), NIQE_FEATURES, dtype=torch.float64, device=a.device)
        ws = torch.empty(nws, dtype=torch.float64, device=a.device)
        A.check(L.srganfd_niqe_features(a.data_ptr(), n, c, h, w, self.crop_border, bh, bw, table.data_ptr(), table.shape[1], feat.data_ptr(),
                                        ws.data_ptr(), A.stream_ptr()), "niqe_features")
        return feat, ws[:n * lh * lw].view(n, lh, lw), ws[n * lh * lw:].view(n, lh // 2, lw // 2)

    def score(self, feat: Tensor) -> Tensor:
        """(N, blocks, 36) fp64 features -> (N,) scores (image_quality_assessment.py:1259-1268, :944-978)"""
        _, mu_p, cov_p = self._on(feat.device)
        nan = torch.isnan(feat)
        mu_d = torch.where(nan, 0.0, feat).sum(1) / (~nan).sum(1)
        keep = ~nan.any(2, keepdim=True)                                  # blocks without a NaN
        rows = keep.sum(1)                                                # (N, 1)
        mean = torch.where(keep, feat, 0.0).sum(1, keepdim=True) / rows.unsqueeze(1)
        d = torch.where(keep, feat - mean, 0.0)
        cov_d = d.transpose(1, 2) @ d / (rows.unsqueeze(1) - 1)
        invcov = torch.linalg.pinv((cov_p + cov_d) / 2, hermitian=self._symmetric)
        diff = (mu_p - mu_d).unsqueeze(1)
        return torch.sqrt(torch.bmm(torch.bmm(diff, invcov), diff.transpose(1, 2)).reshape(-1))

    def forward(self, raw_tensor: Tensor) -> Tensor:
        return self.score(self.features(raw_tensor)[0])
