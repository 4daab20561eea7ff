"""Times model.gen_rpa2x() -- A-ESRGAN's pixel-attention generator, 20 RPA blocks and one US block, on the HIP engine
(sr_gan_fd_amd/engine_rpa.py) -- beside a torch restatement of the same network (F.conv2d / F.interpolate over the same state dict,
the reference's order: up-sampling first), on the same GPU, weights and inputs.
    python tools/rpa_bench.py [--reps 20] [--out profiles/rpa_bench.txt]
Shapes: A-ESRGAN's training shape, LR 60 x 60 at batch 8 (aesrgan_config.py:101-103), and batch 32.  Precisions: f16 (the HIP module
pinned to it, torch under autocast) and fp32.  Rows: forward (no graph) and forward + backward.
Method: 3 warm-up calls per row, then ``reps`` calls timed one by one with device events, the HIP and the torch call alternating;
median (min .. max).  No speed ratio is a pass condition: slower rows are printed as such.
A second pass, profiler on (profiling.REC, every launch bracketed by an event pair), gives the share of the bracketed kernel time per
launch label of forward + backward: pixel_gate, each conv class, the weight gradients.  Not bracketed and so not in that total: the
layout conversions at both ends, srganfd_lrelu_bwd, srganfd_resample and, in fp32, the first layer's data gradient."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sr_gan_fd_amd import model as M  # noqa: E402
from sr_gan_fd_amd import profiling  # noqa: E402

SHAPES = ((8, 60, 60), (32, 60, 60))


def torch_forward(p, x, num_block, num_us):
    """Generator_RPA.forward (A-ESRGAN/model.py:166-175) over a state dict"""
    conv = lambda t, n, pad: F.conv2d(t, p[n + ".weight"], p[n + ".bias"], padding=pad)
    lrelu = lambda t: F.leaky_relu(t, 0.2)
    z = lrelu(conv(x, "conv1", 1))
    cur = z
    for i in range(num_block):
        pre = "rpa.rpa%d." % i
        t = lrelu(conv(lrelu(conv(cur, pre + "conv1", 0)), pre + "conv2", 0))
        t = torch.sigmoid(conv(t, pre + "conv3", 1))
        cur = lrelu(conv(cur * t + cur, pre + "conv4", 1))
    cur = z + cur
    for i in range(num_us):
        pre = "us.us%d." % i
        u = lrelu(conv(F.interpolate(cur, scale_factor=2, mode="nearest"), pre + "conv1", 0))
        t = torch.sigmoid(conv(u, pre + "pa_conv", 0))
        cur = lrelu(conv(u * t + u, pre + "conv2", 1))
    return conv(lrelu(conv(cur, "conv2", 1)), "conv3", 1)


def timed_pair(f_hip, f_torch, reps, warmup=3):
    """both calls, alternating: per call a device-event pair and a synchronise"""
    for _ in range(warmup):
        f_hip()
        f_torch()
    torch.cuda.synchronize()
    times = ([], [])
    for _ in range(reps):
        for fn, ts in zip((f_hip, f_torch), times):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
    return [(statistics.median(t), min(t), max(t)) for t in times]


def label_class(label):
    if label.startswith("pixel_gate"):
        return label
    if label.startswith("wgrad") or "thin_wgrad" in label:
        return "weight gradients (" + label.split("<")[0] + ")"
    return label


def shares(m, x, d, steps):
    rec = profiling.enable(every=1)
    try:
        for _ in range(steps):
            m.zero_grad(set_to_none=True)
            m(x).backward(d)
        agg = profiling.summary(rec)
    finally:
        profiling.disable()
    total = sum(v["ms"] for v in agg.values())
    by = {}
    for label, v in agg.items():
        c = by.setdefault(label_class(label), [0.0, 0])
        c[0] += v["ms"]
        c[1] += v["launches"]
    return total / steps, sorted(((k, ms / total, n // steps, ms / steps) for k, (ms, n) in by.items()), key=lambda r: -r[1])


def rows(reps, emit):
    dev = torch.device("cuda", 0)
    emit(f"device: {torch.cuda.get_device_name(0)}; median (min .. max) of {reps} calls each, device events, 3 warm-up calls, HIP and torch alternating")
    emit("HIP: model.gen_rpa2x() (20 RPA blocks, 1 US block); torch: the same network as F.conv2d / F.interpolate calls over the same state dict")
    torch.manual_seed(0)
    m = M.gen_rpa2x().to(dev)
    params = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    nb, nu = len(m.rpa), len(m.us)
    for n, h, w in SHAPES:
        for name, dt in (("f16", torch.float16), ("fp32", torch.float32)):
            m.compute_dtype = dt
            x = torch.rand(n, 3, h, w, device=dev)
            d = torch.randn(n, 3, 2 * h, 2 * w, device=dev)
            cast = lambda: torch.autocast("cuda", dtype=torch.float16, enabled=dt is torch.float16)

            def hip_fwd():
                with torch.no_grad():
                    return m(x)

            def torch_fwd():
                with torch.no_grad(), cast():
                    return torch_forward(params, x, nb, nu)

            def hip_step():
                m.zero_grad(set_to_none=True)
                m(x).backward(d)

            def torch_step():
                for p in params.values():
                    p.grad = None
                with cast():
                    out = torch_forward(params, x, nb, nu)
                out.backward(d.to(out.dtype))
            a, t = hip_fwd(), torch_fwd().float()
            emit(f"batch {n}, LR {h} x {w}, {name}: outputs agree to {float((a - t).abs().max() / t.abs().max()):.1e} of the maximum")
            for what, fh, ft in (("forward", hip_fwd, torch_fwd), ("forward + backward", hip_step, torch_step)):
                hip, tor = timed_pair(fh, ft, reps)
                note = "" if hip[0] <= tor[0] else "   (the HIP path is SLOWER here)"
                emit(f"  {what:18s} HIP {hip[0]:8.3f} ms ({hip[1]:.3f} .. {hip[2]:.3f})   torch {tor[0]:8.3f} ms ({tor[1]:.3f} .. {tor[2]:.3f})   "
                     f"torch / HIP {tor[0] / hip[0]:6.2f} x{note}")
            step_ms = hip[0]
            total, table = shares(m, x, d, 3)
            emit(f"  forward + backward, profiler on: {total:.3f} ms of bracketed kernel time per step (the step above, profiler off: {step_ms:.3f} ms)")
            for label, share, launches, ms in table:
                emit(f"    {100 * share:5.1f} %  {ms:8.3f} ms  {launches:4d} launches  {label}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    out = open(args.out, "w") if args.out else None

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    rows(args.reps, emit)
    if out:
        out.close()


if __name__ == "__main__":
    main()
