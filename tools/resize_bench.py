"""Times imgproc.image_resize (srganfd_imresize) on the GPU beside its nearest relative, imgproc.interpolate(mode="bicubic")
(srganfd_resize mode 2: 16 taps, no antialiasing, torch's coordinate rule), at the same input and output shapes.
    python tools/resize_bench.py [--reps 30] [--inner 10] [--out profiles/imresize_kernel_stats.txt]
One sample = device events around `inner` launches in a row, divided by `inner`; the figure is the median of `reps` samples after a
warm-up, the two functions alternating sample by sample.  Each launch reads another input of a ring of buffers that together exceed
the 256 MB Infinity Cache where the shape allows (at most 8 buffers), so the large shape is read from HBM, not from the cache the
previous launch filled.  Bytes are the algorithm's: every input float read once, every output float written once."""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sr_gan_fd_amd import _abi as A  # noqa: E402
from sr_gan_fd_amd import imgproc  # noqa: E402

SHAPES = (((32, 3, 512, 512), 1 / 4), ((16, 3, 128, 128), 1 / 4), ((32, 3, 128, 128), 4))


def sample_ms(launch, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(inner):
        launch(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    assert args.reps * args.inner >= 20
    dev = torch.device("cuda", 0)
    L = A.lib()
    lines = [f"device: {torch.cuda.get_device_name(0)}; per launch: median (min .. max) of {args.reps} samples of {args.inner} launches in a row, "
             "device events, 3 warm-up samples; GB/s = (input + output bytes) / median"]
    for shape, scale in SHAPES:
        n, c, h, w = shape
        oh, ow = math.ceil(h * scale), math.ceil(w * scale)
        nbytes = 4 * n * c * (h * w + oh * ow)
        ring = max(1, min(8, math.ceil(512e6 / (4 * n * c * h * w))))
        torch.manual_seed(0)
        xs = [torch.rand(*shape, device=dev) for _ in range(ring)]
        out = torch.empty(n, c, oh, ow, device=dev)
        wt_h, first_h, taps_h = imgproc._resize_tables(h, oh, scale, True, "height", dev)
        wt_w, first_w, taps_w = imgproc._resize_tables(w, ow, scale, True, "width", dev)
        st = torch.cuda.current_stream().cuda_stream
        rs = float(1.0 / scale)

        def new(i):      # the entry points themselves: no allocation, no table lookup in the timed window
            A.check(L.srganfd_imresize(xs[i % ring].data_ptr(), n * c, h, w, oh, ow, wt_h.data_ptr(), first_h.data_ptr(), taps_h, wt_w.data_ptr(),
                                       first_w.data_ptr(), taps_w, out.data_ptr(), st), "imresize")

        def old(i):
            A.check(L.srganfd_resize(xs[i % ring].data_ptr(), n * c, h, w, oh, ow, 2, rs, rs, out.data_ptr(), st), "resize")

        assert imgproc.image_resize(xs[0], scale).shape == out.shape and imgproc.interpolate(xs[0], scale_factor=scale, mode="bicubic").shape == out.shape
        t = {"new": [], "old": []}
        for r in range(args.reps + 3):
            a, b = sample_ms(new, args.inner), sample_ms(old, args.inner)
            if r >= 3:
                t["new"].append(a)
                t["old"].append(b)
        lines.append(f"input {shape} x {scale:g} -> {oh} x {ow}: {nbytes / 1e6:.1f} MB, ring of {ring} inputs, {taps_h} taps per pass")
        for key, name in (("new", "srganfd_imresize (image_resize)"), ("old", "srganfd_resize mode 2 (interpolate bicubic)")):
            med = statistics.median(t[key])
            lines.append(f"  {name:44s} {med * 1e3:9.1f} us ({min(t[key]) * 1e3:.1f} .. {max(t[key]) * 1e3:.1f})   {nbytes / (med * 1e-3) / 1e9:7.0f} GB/s")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
