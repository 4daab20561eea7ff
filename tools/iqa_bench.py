"""Times the validation metrics (NIQE, SSIM, PSNR) on the GPU: warm-up, device events around each call, median of the repetitions.
    python tools/iqa_bench.py [--reps 30] [--out profiles/iqa_times.txt]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
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
