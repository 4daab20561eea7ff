#!/usr/bin/env python3
"""Throughput of the on-device degradation stages at Real-ESRGAN's training shape (batch 48, 3x256x256 GT,
realesrgan_config.py:116-117), each stage against the roof that bounds it, plus the whole degradation_process (the CPU side of
the comparison is bench.py's cpu_baseline leg of `--workload realesrgan_gan`; the oracle is not used from tools/).

    python tools/degrade_bench.py [--batch 48] [--size 256] [--iters 20]
    python tools/degrade_bench.py --bsrgan [--batch 32] [--size 512] [--iters 20]
    python tools/degrade_bench.py --digest      one sha1 per entry point on seeded inputs; run once per build (SRGANFD_LIB=<other build>, a fresh
                                                process each) and compare the lines: equal bits iff all agree

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


def digests():
    """one sha1 per entry point of csrc/filter2d.hip, jpeg.hip and degrade.hip on seeded inputs, at every size where a kernel takes another
    path (ragged tiles, the mirror limit, a dead wave, a copied-through image): two builds compute the same bits iff every line agrees"""
    from tools.ewbench import digest
    imgproc = importlib.import_module("sr_gan_fd_amd.imgproc")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    rand = lambda *s, dtype=torch.float32: torch.rand(*s, device="cuda", generator=gen, dtype=dtype)
    randn = lambda *s: torch.randn(*s, device="cuda", generator=gen)

    def row(name, *outs):
        torch.cuda.synchronize()
        print(f"{name:58s} " + " ".join(digest(o) for o in outs), flush=True)

    def kernels(n, k, dtype=torch.float32):
        kk = rand(n, k, k, dtype=dtype)
        return kk / kk.sum(dim=(1, 2), keepdim=True)
    for h, w, ks in ((32, 64, (3, 21, 51)), (33, 65, (3, 21, 51)), (100, 130, (3, 21, 51)), (27, 26, (51,))):
        x = rand(2, 3, h, w)
        for k in ks:
            row(f"filter2d {h}x{w} k={k} shared / per-image", imgproc.filter2d_torch(x, kernels(1, k)), imgproc.filter2d_torch(x, kernels(2, k)))
    x, taps = rand(2, 3, 50, 90), rand(2, 18)
    out = torch.empty_like(x)
    A = importlib.import_module("sr_gan_fd_amd._abi")
    A.check(A.lib().srganfd_filter2d_separable(x.data_ptr(), taps.data_ptr(), 2, 2, 3, 50, 90, 9, out.data_ptr(), A.stream_ptr()), "filter2d_separable")
    row("filter2d_separable 50x90 per-image 9 taps", out)
    usm, usm_full = imgproc.USMSharp().cuda(), imgproc.USMSharp().cuda()
    usm_full.kernel.copy_(kernels(1, 51))                                    # not an outer product: the rank-51 path
    for n in (64, 256):
        x = rand(2, 3, n, n)
        row(f"usm_sharp {n}x{n} separable / rank-51", usm(x, 0.5, 10), usm_full(x, 0.5, 10))
    for h, w in ((33, 65), (512, 512)):
        k25 = torch.zeros(3, 25, 25, device="cuda", dtype=torch.float64)
        k25[1, 9:16, 9:16], k25[2] = kernels(1, 7, torch.float64)[0], kernels(1, 25, torch.float64)[0]
        row(f"filter2d_mirror_f64 {h}x{w} k = 0 / 7 / 25", imgproc.filter2d_mirror_f64(rand(3, 3, h, w), k25, [0, 7, 25]))
    jpeg, jpeg_d = imgproc.DiffJPEG().cuda(), imgproc.DiffJPEG(differentiable=True).cuda()
    for b, h, w in ((1, 16, 16), (1, 17, 15), (1, 130, 33), (3, 16, 16), (48, 256, 256)):
        x = rand(b, 3, h, w)
        q = rand(b) * 65 + 30
        row(f"diff_jpeg {b}x3x{h}x{w} round / cubic", jpeg(x, q.clone()), jpeg_d(x, q.clone()))
        row(f"jpeg_roundtrip {b}x3x{h}x{w} q = 1 / 50 / 100", *[imgproc.jpeg_compression(x, q) for q in (1, 50, 100)])
        if b == 3:
            row(f"jpeg_roundtrip {b}x3x{h}x{w} q = 40, 0, 90", imgproc.jpeg_compression(x, [40, 0, 90]))
    x = rand(4, 3, 100, 130) * 1.2 - 0.1
    row("quantize_u8", imgproc.quantize_u8(x))
    for mode in ("area", "bilinear", "bicubic"):
        row(f"resize {mode} x1.37 / x0.41 / -> 64x48", imgproc.interpolate(x, scale_factor=1.37, mode=mode), imgproc.interpolate(x, scale_factor=0.41, mode=mode),
            imgproc.interpolate(x, size=(64, 48), mode=mode))
    sigma, gray = rand(4) * 30, torch.tensor([0., 1., 0., 1.], device="cuda")
    n_color, n_gray = randn(4, 3, 100, 130), randn(100, 130)
    row("gaussian_noise colour / grey", imgproc.gaussian_noise_apply(x, n_color, None, sigma, gray, False, False),
        imgproc.gaussian_noise_apply(x, n_color, n_gray, sigma, gray, False, False))
    row("gaussian_noise clip x rounds", *[imgproc.gaussian_noise_apply(x, n_color, n_gray, sigma, gray, c, r) for c in (False, True) for r in (False, True)])
    for want_gray in (False, True):
        img_q, gray_q, vals, vals_gray = imgproc.poisson_noise_prepare(x, want_gray)
        row(f"poisson_prepare grey = {want_gray}", *[t for t in (img_q, gray_q, vals, vals_gray) if t is not None])
        pois = torch.floor(img_q * vals.view(4, 1, 1, 1) + randn(4, 3, 100, 130))             # any draw does: the apply stage is deterministic
        pois_g = torch.floor(gray_q * vals_gray.view(4, 1, 1, 1) + randn(4, 1, 100, 130)) if want_gray else None
        row(f"poisson_apply grey = {want_gray} clip x rounds", *[imgproc.poisson_noise_apply(x, img_q, gray_q, pois, pois_g, vals, vals_gray, sigma / 10,
                                                                                            gray if want_gray else None, c, r) for c in (False, True) for r in (False, True)])
    sq = rand(2, 3, 96, 96)
    row("crop_rot_flip ops 0 .. 5", *[imgproc._crop_rot_flip(sq, 5, 7, 64, 64, op) for op in range(6)])
    gt, k21 = rand(4, 3, 256, 256), kernels(4, 21)
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    imgproc.DRAW_DEVICE = "cpu"                                              # the draws come from the seeded host generators: the same on every build
    row("degradation_process (seeded draws)", *imgproc.degradation_process(gt, k21, k21, k21, 4, PARAMS, jpeg, usm))
    draws = imgproc.bsrgan_degradation_draws(4, 4)
    row("degradation_process_bsrgan (recorded draws)", imgproc.degradation_process_bsrgan(gt, 4, draws=draws))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--size", type=int, default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--bsrgan", action="store_true")
    ap.add_argument("--digest", action="store_true")
    a = ap.parse_args()
    if a.digest:
        return digests()
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
