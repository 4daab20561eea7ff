"""Times the validation metrics (NIQE, SSIM, PSNR) on the GPU: warm-up, device events around each call, median of the repetitions.
    python tools/iqa_bench.py [--reps 30] [--out profiles/iqa_times.txt]
    python tools/iqa_bench.py --lpips [--reps 30] [--out profiles/lpips_bench.txt]      the LPIPS row, see lpips_rows()
Inputs: 16 x 3 x 512 x 512 and one DIV2K-sized 1 x 3 x 1356 x 2040 image, the same tensors for the three metrics.  NIQE's bytes/s
counts what its kernels must move: three float32 planes read, the fp64 luma plane written and read twice (scale-1 blocks, resize),
the fp64 half-size plane written and read once.  NIQE uses a synthetic model (the time does not depend on its values)."""
import argparse
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sr_gan_fd_amd.image_quality_assessment import NIQE, PSNR, SSIM  # noqa: E402


def median_ms(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def torch_lpips(sd):
    """the same network composed from torch's own GPU ops in fp32 (what the `lpips` package runs): in0 and in1 as one 2N batch"""
    import torch.nn.functional as F
    convs = [(sd[f"net.slice{i + 1}.{k}.weight"], sd[f"net.slice{i + 1}.{k}.bias"], st, pd, pool)
             for i, (k, st, pd, pool) in enumerate((("0", 4, 2, False), ("3", 1, 2, True), ("6", 1, 1, True), ("8", 1, 1, False), ("10", 1, 1, False)))]
    lins = [sd[f"lin{i}.model.1.weight"] for i in range(5)]
    shift, scale = sd["scaling_layer.shift"], sd["scaling_layer.scale"]

    def run(in0, in1):
        n = in0.shape[0]
        x = (torch.cat([in0, in1]) - shift) / scale
        total = 0
        for (w, b, st, pd, pool), lin in zip(convs, lins):
            if pool:
                x = F.max_pool2d(x, 3, 2)
            x = F.relu(F.conv2d(x, w, b, stride=st, padding=pd))
            f = x / (torch.sqrt(torch.sum(x * x, dim=1, keepdim=True)) + 1e-10)
            total = total + F.conv2d((f[:n] - f[n:]) ** 2, lin).mean(dim=(2, 3), keepdim=True)
        return total
    return run


def device_kernels(fn):
    """device kernels one call launches, counted by torch's profiler; None where the profiler gives no device events"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        count = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return count or None
    except Exception:      # a tool: the timing rows do not depend on the profiler
        return None


def lpips_rows(reps):
    """LPIPS (5 conv launches + 2 head launches in HIP) beside torch's own fp32 ops, at the validation shape and a batch shape"""
    import warnings
    from sr_gan_fd_amd.image_quality_assessment import LPIPS
    dev = torch.device("cuda", 0)
    torch.backends.cudnn.allow_tf32 = False
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = LPIPS(net="alex").to(dev)
    ref = torch_lpips({k: v.to(dev) for k, v in m.state_dict().items()})
    lines = [f"device: {torch.cuda.get_device_name(0)}; median (min .. max) of {reps} calls, device events, 5 warm-up calls; fp32; seeded weights",
             "HIP: sr_gan_fd_amd LPIPS, 7 launches per call (5 convs with both max-pools folded into the gather, head, finish)",
             "torch: the same network from F.conv2d / F.max_pool2d / elementwise ops on the 2N batch"]
    for shape in ((1, 3, 512, 512), (16, 3, 128, 128)):
        torch.manual_seed(0)
        gt = torch.rand(*shape, device=dev)
        sr = (gt + 0.1 * torch.randn_like(gt)).clamp(0, 1)
        a, b = m(sr, gt), ref(sr, gt)
        diff = ((a - b).abs() / b.abs()).max().item()
        hip, tor = median_ms(lambda: m(sr, gt), reps), median_ms(lambda: ref(sr, gt), reps)
        k_hip, k_tor = device_kernels(lambda: m(sr, gt)), device_kernels(lambda: ref(sr, gt))
        lines.append(f"input {shape}: HIP and torch agree to {diff:.1e} relative")
        lines.append(f"  LPIPS HIP    {hip[0]:8.3f} ms ({hip[1]:.3f} .. {hip[2]:.3f})   device kernels per call (profiler): {k_hip}")
        lines.append(f"  LPIPS torch  {tor[0]:8.3f} ms ({tor[1]:.3f} .. {tor[2]:.3f})   device kernels per call (profiler): {k_tor}")
        lines.append(f"  torch / HIP  {tor[0] / hip[0]:8.2f} x" + ("" if hip[0] < tor[0] else "   (the HIP path is NOT faster here)"))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lpips", action="store_true", help="time LPIPS beside torch's own ops instead of the NIQE / SSIM / PSNR rows")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    if args.lpips:
        text = "\n".join(lpips_rows(args.reps))
        print(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    from scipy.io import savemat
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(0)
    q, _ = np.linalg.qr(rng.normal(size=(36, 36)))
    lines = [f"device: {torch.cuda.get_device_name(0)}; median (min .. max) of {args.reps} calls, device events, 5 warm-up calls"]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "niqe_model.mat")
        savemat(path, {"mu_prisparam": rng.uniform(size=(1, 36)), "cov_prisparam": (q * rng.uniform(0.1, 2.0, size=36)) @ q.T})
        niqe, ssim, psnr = NIQE(4, path), SSIM(4, True), PSNR(4, True)
        for shape in ((16, 3, 512, 512), (1, 3, 1356, 2040)):
            torch.manual_seed(0)
            sr = torch.rand(*shape, device=dev)
            gt = (sr + 0.05 * torch.randn_like(sr)).clamp(0, 1)
            n, _, h, w = shape
            lh, lw = (h - 8) // 96 * 96, (w - 8) // 96 * 96
            nbytes = n * (12 * h * w + 3 * 8 * lh * lw + 2 * 8 * (lh // 2) * (lw // 2))
            feat = niqe.features(sr)[0]
            rows = (("NIQE", lambda: niqe(sr)), ("NIQE features (4 HIP launches)", lambda: niqe.features(sr)),
                    ("NIQE score (36 x 36 torch ops)", lambda: niqe.score(feat)), ("SSIM", lambda: ssim(sr, gt)), ("PSNR", lambda: psnr(sr, gt)))
            lines.append(f"input {shape}:")
            for name, fn in rows:
                med, lo, hi = median_ms(fn, args.reps)
                extra = f"   {nbytes / (med * 1e-3) / 1e9:.0f} GB/s over {nbytes / 1e6:.1f} MB" if name.startswith("NIQE features") else ""
                lines.append(f"  {name:32s} {med:8.3f} ms ({lo:.3f} .. {hi:.3f}){extra}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
