#!/usr/bin/env python3
"""Throughput of the on-device degradation stages at Real-ESRGAN's training shape (batch 48, 3x256x256 GT,
realesrgan_config.py:116-117), each stage against the roof that bounds it, plus the whole degradation_process (the CPU side of
the comparison is bench.py's cpu_baseline leg of `--workload realesrgan_gan`; the oracle is not used from tools/).

    python tools/degrade_bench.py [--batch 48] [--size 256] [--iters 20]
    python tools/degrade_bench.py --bsrgan [--batch 32] [--size 512] [--iters 20]

--bsrgan: BSRGAN's blind degradation (imgproc.degradation_process_bsrgan) at the headline shape (batch 32, 3x512x512 GT, factor 4): the
whole call on fresh draws (host clock around a device synchronise: the draws and the kernel synthesis on the host are part of it), its two
kernels alone (the JPEG round trip; the fp64 blur at k = 25 with the fp32 srganfd_filter2d at k = 25 beside it, so the price of fp64 is a
measured number), and -- where scipy and Pillow import -- the same per-image program on the host (scipy's convolve, Pillow's JPEG, the
tests' resize oracle: the only way to make these LR images without this library), with the ratio.

Prints one JSON line per stage: {"stage", "us", "GB/s" (algorithmic bytes: input read once + output written once),
"hbm_frac" (of 8 TB/s), "GFLOP/s", "valu_frac" (of 157.3 TFLOP/s fp32 vector)}.  Timed with HIP events on the current stream.
"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import importlib

PEAK_HBM, PEAK_VALU = 8000e9, 157.3e12
PARAMS = dict(first_blur_probability=1.0, resize_probability1=[0.2, 0.7, 0.1], resize_range1=[0.15, 1.5], gray_noise_probability1=0.4,
              gaussian_noise_probability1=0.5, noise_range1=[1, 30], poisson_scale_range1=[0.05, 3], jpeg_range1=[30, 95],
              second_blur_probability=0.8, resize_probability2=[0.3, 0.4, 0.3], resize_range2=[0.3, 1.2], gray_noise_probability2=0.4,
              gaussian_noise_probability2=0.5, noise_range2=[1, 25], poisson_scale_range2=[0.05, 2.5], jpeg_range2=[30, 95])


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


def host_degrade(gt, rec, kernels):
    """one image's program on the host with the libraries the reference uses for it (cv2's JPEG is libjpeg, as Pillow's is)"""
    import io
    from PIL import Image
    from scipy import ndimage
    from tests import bsrgan_degradation_oracle as BO, resize_oracle as RO

    def jpeg(x, q):
        u8 = np.uint8((x.clip(0, 1) * np.float32(255.)).round()).transpose(1, 2, 0)
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(u8)).save(buf, format="JPEG", quality=q)
        return (np.float32(np.array(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))) / np.float32(255.)).transpose(2, 0, 1)

    x, nb = BO.half_step(gt, rec), 0
    for kind, p in rec["ops"]:
        if kind == "blur":
            x = ndimage.convolve(x, BO.trim_kernel(kernels[nb], p["ksize"])[None], mode="mirror")
            nb += 1
        elif p:
            x = jpeg(x, p)
    return RO.resize(jpeg(x, rec["final_quality"]), 1 / rec["sf"], True)


def bsrgan(a):
    import time
    imgproc = importlib.import_module("sr_gan_fd_amd.imgproc")
    b, n = a.batch or 32, a.size or 512
    torch.manual_seed(0)
    random.seed(0); np.random.seed(0)
    gt = torch.rand(b, 3, n, n, device="cuda")
    img_bytes, px = gt.numel() * 4, b * 3 * n * n
    out = lambda d: print(json.dumps(d), flush=True)

    def whole():
        for _ in range(3):
            imgproc.degradation_process_bsrgan(gt, 4)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            imgproc.degradation_process_bsrgan(gt, 4)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.iters
    t_all = whole()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        imgproc.bsrgan_blur_kernels(imgproc.bsrgan_degradation_draws(b, 4), 4)
    t_host = (time.perf_counter() - t0) / a.iters
    out({"stage": "degradation_process_bsrgan (fresh draws every call, host clock + synchronise)", "ms": round(t_all * 1e3, 3), "img/s": round(b / t_all, 1),
         "of which draws + kernel synthesis on the host, ms": round(t_host * 1e3, 3), "batch": b, "gt": f"3x{n}x{n}", "factor": 4})
    q = torch.full((b,), 60, dtype=torch.int32, device="cuda")
    q_host = np.full(b, 60, dtype=np.int32)
    t = timed(lambda: imgproc._jpeg_roundtrip(gt, q, q_host), a.iters)
    out({"stage": "srganfd_jpeg_roundtrip q = 60 (two launches)", "us": round(t * 1e6, 1), "GB/s": round((2 * img_bytes + 2 * 1.5 * px / 3) / t / 1e9, 1),
         "hbm_frac": round((2 * img_bytes + 2 * 1.5 * px / 3) / t / PEAK_HBM, 4)})
    k25 = torch.rand(b, 25, 25, device="cuda", dtype=torch.float64)
    k25 = k25 / k25.sum(dim=(1, 2), keepdim=True)
    k25f = k25.float()
    for k in (25, 15, 7):
        ks_host = np.full(b, k, dtype=np.int32)
        ks = torch.from_numpy(ks_host).cuda()
        t64 = timed(lambda: imgproc._filter2d_mirror_f64(gt, k25, ks, ks_host), a.iters)
        o = (25 - k) // 2
        kf = k25f[:, o:o + k, o:o + k].contiguous()
        t32 = timed(lambda: imgproc.filter2d_torch(gt, kf), a.iters)
        out({"stage": f"blur k = {k}: srganfd_filter2d_mirror_f64 (fp64 FMA) vs srganfd_filter2d (fp32)", "fp64 us": round(t64 * 1e6, 1), "fp32 us": round(t32 * 1e6, 1),
             "fp64 / fp32": round(t64 / t32, 2), "fp64 GFMA/s": round(px * k * k / t64 / 1e9, 1), "fp64_valu_frac (of 78.6 TFLOP/s)": round(2.0 * px * k * k / t64 / 78.6e12, 4)})
    try:
        import PIL, scipy  # noqa: F401
    except ImportError as e:
        out({"stage": "host path", "skipped": f"{e}"})
        return
    random.seed(1); np.random.seed(1)
    m = min(b, 4)
    draws = imgproc.bsrgan_degradation_draws(m, 4)
    kernels, _ = imgproc.bsrgan_blur_kernels(draws, 4)
    g = gt[:m].cpu().numpy()
    t0 = time.perf_counter()
    for i in range(m):
        host_degrade(g[i], draws[i], kernels[i])
    t_cpu = (time.perf_counter() - t0) / m
    out({"stage": "the same program on the host (scipy convolve, Pillow JPEG, fp64 resize oracle), one process", "ms per image": round(t_cpu * 1e3, 1),
         "ms per batch": round(t_cpu * b * 1e3, 1), "host / device": round(t_cpu * b / t_all, 1)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--size", type=int, default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--bsrgan", action="store_true")
    a = ap.parse_args()
    if a.bsrgan:
        return bsrgan(a)
    a.batch, a.size = a.batch or 48, a.size or 256
    imgproc = importlib.import_module("sr_gan_fd_amd.imgproc")
    b, n = a.batch, a.size
    torch.manual_seed(0)
    gt = torch.rand(b, 3, n, n, device="cuda")
    k21 = torch.rand(b, 21, 21, device="cuda")
    k21 = k21 / k21.sum(dim=(1, 2), keepdim=True)
    usm, jpeg = imgproc.USMSharp().cuda(), imgproc.DiffJPEG().cuda()
    img_bytes = gt.numel() * 4
    px = b * 3 * n * n
    quality = torch.full((b,), 60.0, device="cuda")
    randn = torch.randn_like(gt)
    sigma, gray = torch.full((b,), 10.0, device="cuda"), torch.zeros(b, device="cuda")
    stages = [
        ("filter2d 21x21 per-image kernels", lambda: imgproc.filter2d_torch(gt, k21), 2 * img_bytes, 2.0 * px * 441),
        ("USMSharp 51x51 (two fused separable passes)", lambda: usm(gt, 0.5, 10), 7 * img_bytes, 2.0 * px * (51 * 82 / 32 + 51) * 2),
        ("DiffJPEG round trip", lambda: jpeg(gt, quality.clone()), 2 * img_bytes, 2.0 * px * 64 * 2 * 1.5),
        ("resize bicubic x0.5", lambda: imgproc.interpolate(gt, scale_factor=0.5, mode="bicubic"), 1.25 * img_bytes, 2.0 * px / 4 * 20),
        ("resize area -> 64x64", lambda: imgproc.interpolate(gt, size=(n // 4, n // 4), mode="area"), (1 + 1 / 16) * img_bytes, px),
        ("gaussian noise apply (draws given)", lambda: imgproc.gaussian_noise_apply(gt, randn, None, sigma, gray, True, False), 3 * img_bytes, 3.0 * px),
        ("quantize_u8", lambda: imgproc.quantize_u8(gt), 2 * img_bytes, 3.0 * px),
    ]
    for name, fn, nbytes, flop in stages:
        t = timed(fn, a.iters)
        print(json.dumps({"stage": name, "us": round(t * 1e6, 1), "GB/s": round(nbytes / t / 1e9, 1), "hbm_frac": round(nbytes / t / PEAK_HBM, 4),
                          "GFLOP/s": round(flop / t / 1e9, 1), "valu_frac": round(flop / t / PEAK_VALU, 4)}))

    def pipeline():
        return imgproc.degradation_process(gt, k21, k21, k21, 4, PARAMS, jpeg, usm)
    random.seed(0); np.random.seed(0)
    t = timed(pipeline, a.iters)
    line = {"stage": "degradation_process (USM + 2nd-order pipeline, random branches)", "ms": round(t * 1e3, 3), "img/s": round(b / t, 1),
            "batch": b, "gt": f"3x{n}x{n}"}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
