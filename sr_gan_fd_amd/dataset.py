"""Device-side batch prefetching with the interface the train loops use (reference: BSRGAN/dataset.py:203-243,
``CUDAPrefetcher``: ``next()`` / ``reset()`` / ``len()``; batches are dicts of tensors, e.g. {"gt": ..., "lr": ...}).

The HIP kernels run on torch's current stream; the prefetcher stages the NEXT batch on its own copy stream and makes the
current stream wait for that copy before handing the batch over, so the host-to-device transfer of batch i+1 overlaps the
training iteration on batch i.  Tensors handed out are recorded on the consumer stream so the caching allocator does not
recycle them while kernels launched through the C ABI (which torch cannot see) may still read them.
"""
from __future__ import annotations

import torch


class CUDAPrefetcher:
    """``ingest_u8`` (an addition; the reference's loader hands out fp32 CHW tensors): a batch entry that is a uint8 (N, H, W, 3) tensor -- decoded
    images as cv2.imread returns them -- is copied as bytes and converted on the device on the copy stream (imgproc.image_to_tensor_u8:
    / 255, BGR -> RGB, HWC -> CHW), so the consumer sees the same fp32 (N, 3, H, W) batch at a quarter of the PCIe traffic.

    ``synthesize_lr`` (an addition; ESRGAN/dataset.py:73 makes the LR image per sample on the host with ``imgproc.image_resize(gt_image,
    1 / upscale_factor)``): with an upscale factor, a batch that has ``"gt"`` and no ``"lr"`` gets ``batch["lr"] = image_resize(batch["gt"],
    1 / factor)`` on the copy stream, after the u8 ingest, so the resize of batch i+1 overlaps iteration i like the copy does.  A batch that
    brings its own ``"lr"`` keeps it; the default ``None`` changes nothing.  (The reference resizes in BGR and swaps channels afterwards; the
    resize is per channel, so the order does not matter.)

    ``synthesize_lr_bsrgan`` (an addition; BSRGAN/dataset.py:83 and A-ESRGAN's make the LR image per sample on the host with
    ``imgproc.degradation_process(gt, upscale_factor, jpeg_prob, scale2_prob)`` in cv2, scipy and numpy): a dict with ``upscale_factor`` and
    optionally ``jpeg_prob`` / ``scale2_prob``; a batch that has ``"gt"`` and no ``"lr"`` gets ``batch["lr"] =
    imgproc.degradation_process_bsrgan(batch["gt"], **dict)`` on the copy stream, the random draws taken from the global ``random`` /
    ``np.random`` streams when the batch is staged.  It excludes ``synthesize_lr`` (``ValueError``): a batch gets one LR.

    ``synthesize_kernels_realesrgan`` (an addition; Real_ESRGAN/dataset.py:64-133 makes three filter kernels per sample on the host with
    ``imgproc.random_mixed_kernels`` / ``generate_sinc_kernel`` in numpy and scipy): the degradation-model parameter dict
    (realesrgan_config.py:46-65); a batch that has ``"gt"`` and no ``"gaussian_kernel1"`` gets ``"gaussian_kernel1"``,
    ``"gaussian_kernel2"`` and ``"sinc_kernel"`` from ``imgproc.realesrgan_kernel_draws`` (the global ``random`` / ``np.random`` streams,
    when the batch is staged) and ``imgproc.realesrgan_blur_kernels`` (one launch on the copy stream), so the dataset returns ``"gt"``
    only.  A batch that brings its own kernels keeps them; a dict that lacks a key raises ``ValueError`` here, naming it."""

    def __init__(self, dataloader, device: torch.device, ingest_u8: bool = False, bgr: bool = True, synthesize_lr: int | None = None,
                 synthesize_lr_bsrgan: dict | None = None, synthesize_kernels_realesrgan: dict | None = None):
        self.original_dataloader = dataloader
        self.ingest_u8, self.bgr = ingest_u8, bgr
        if synthesize_lr is not None and not synthesize_lr >= 1:
            raise ValueError(f"CUDAPrefetcher: synthesize_lr is the upscale factor (>= 1) or None, got {synthesize_lr}")
        self.synthesize_lr = synthesize_lr
        if synthesize_lr_bsrgan is not None:
            if synthesize_lr is not None:
                raise ValueError("CUDAPrefetcher: synthesize_lr and synthesize_lr_bsrgan both make batch['lr']; pass one of them")
            unknown = set(synthesize_lr_bsrgan) - {"upscale_factor", "jpeg_prob", "scale2_prob"}
            if "upscale_factor" not in synthesize_lr_bsrgan or unknown:
                raise ValueError("CUDAPrefetcher: synthesize_lr_bsrgan is dict(upscale_factor=..., jpeg_prob=..., scale2_prob=...), got "
                                 f"{sorted(synthesize_lr_bsrgan)}")
            synthesize_lr_bsrgan = dict(synthesize_lr_bsrgan)
        self.synthesize_lr_bsrgan = synthesize_lr_bsrgan
        if synthesize_kernels_realesrgan is not None:
            from .imgproc import check_realesrgan_kernel_parameters
            check_realesrgan_kernel_parameters(synthesize_kernels_realesrgan)
            synthesize_kernels_realesrgan = dict(synthesize_kernels_realesrgan)
        self.synthesize_kernels_realesrgan = synthesize_kernels_realesrgan
        self.device = torch.device(device)
        self.stream = torch.cuda.Stream(device=self.device)
        self.batch_data = None
        self.data = None
        self.reset()

    def _stage(self) -> None:
        try:
            batch = next(self.data)
        except StopIteration:
            self.batch_data = None
            return
        with torch.cuda.stream(self.stream):
            self.batch_data = {k: (v.to(self.device, non_blocking=True) if torch.is_tensor(v) else v) for k, v in batch.items()}
            if self.ingest_u8:
                from .imgproc import image_to_tensor_u8
                for k, v in self.batch_data.items():
                    if torch.is_tensor(v) and v.dtype == torch.uint8 and v.dim() == 4 and v.shape[-1] == 3:
                        self.batch_data[k] = image_to_tensor_u8(v, bgr=self.bgr)      # launched on the copy stream (A.stream_ptr() = current stream)
            if self.synthesize_lr is not None and "lr" not in self.batch_data and torch.is_tensor(self.batch_data.get("gt")):
                from .imgproc import image_resize
                self.batch_data["lr"] = image_resize(self.batch_data["gt"], 1 / self.synthesize_lr)
            if self.synthesize_lr_bsrgan is not None and "lr" not in self.batch_data and torch.is_tensor(self.batch_data.get("gt")):
                from .imgproc import degradation_process_bsrgan
                self.batch_data["lr"] = degradation_process_bsrgan(self.batch_data["gt"], **self.synthesize_lr_bsrgan)
            if (self.synthesize_kernels_realesrgan is not None and "gaussian_kernel1" not in self.batch_data
                    and torch.is_tensor(self.batch_data.get("gt"))):
                from .imgproc import realesrgan_blur_kernels, realesrgan_kernel_draws
                P = self.synthesize_kernels_realesrgan
                draws = realesrgan_kernel_draws(self.batch_data["gt"].shape[0], P)
                kernels = realesrgan_blur_kernels(draws, P, self.device)
                self.batch_data.update(zip(("gaussian_kernel1", "gaussian_kernel2", "sinc_kernel"), kernels))

    def next(self):
        """the staged batch (or None at the end of the epoch); starts staging the following one"""
        consumer = torch.cuda.current_stream(self.device)
        consumer.wait_stream(self.stream)
        batch = self.batch_data
        if batch is not None:
            for v in batch.values():
                if torch.is_tensor(v) and v.is_cuda:
                    v.record_stream(consumer)
        self._stage()
        return batch

    def reset(self) -> None:
        self.data = iter(self.original_dataloader)
        self._stage()

    def __len__(self) -> int:
        return len(self.original_dataloader)
