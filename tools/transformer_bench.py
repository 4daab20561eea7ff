"""Times model.TransformerEncoder -- the reference's transformer block, two post-norm layers of d_model 64, 4 heads, hidden 2048, on
the HIP engine (sr_gan_fd_amd/transformer.py) -- beside torch's nn.TransformerEncoder with the same state dict, on the same GPU and
inputs, at the shape the reference's training script gives it: (8, 900, 64) -- 8 images, 30 x 30 pixel positions.
    python tools/transformer_bench.py [--reps 20] [--out profiles/transformer_bench.txt]
Precisions: f16 (the HIP module pinned to it, torch under autocast) and fp32.  Rows: forward (no graph) and forward + backward, in
eval mode and in train mode (p = 0.1: the four dropout sites live; the two sides draw different masks).
Method: 3 warm-up calls per row, then ``reps`` calls timed one by one with device events, the HIP and the torch call alternating;
median (min .. max).  No speed ratio is a pass condition: the block is under 1 % of its generator's FLOPs, and slower rows are printed
as such.  A second pass, profiler on (profiling.REC, every bracketed launch between an event pair), gives the share of the bracketed
kernel time per launch label of forward + backward; the dtype conversions at both ends are not bracketed."""
import argparse
import os
import statistics
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sr_gan_fd_amd import model as M  # noqa: E402
from sr_gan_fd_amd import profiling  # noqa: E402

SHAPE = (8, 900, 64)


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
    return total / steps, sorted(((k, v["ms"] / total, v["launches"] // steps, v["ms"] / steps) for k, v in agg.items()), key=lambda r: -r[1])


def rows(reps, emit):
    dev = torch.device("cuda", 0)
    emit(f"device: {torch.cuda.get_device_name(0)}; median (min .. max) of {reps} calls each, device events, 3 warm-up calls, HIP and torch alternating")
    emit(f"HIP: model.TransformerEncoder(TransformerEncoderLayer(64, 4), 2); torch: nn.TransformerEncoder over the same state dict; src {SHAPE}")
    torch.manual_seed(0)
    m = M.TransformerEncoder(M.TransformerEncoderLayer(SHAPE[2], 4), 2).to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t = torch.nn.TransformerEncoder(torch.nn.TransformerEncoderLayer(SHAPE[2], 4), 2, enable_nested_tensor=False).to(dev)
    t.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()})
    x = torch.randn(*SHAPE, device=dev)
    d = torch.randn(*SHAPE, device=dev)
    for name, dt in (("f16", torch.float16), ("fp32", torch.float32)):
        m.compute_dtype = dt
        cast = lambda: torch.autocast("cuda", dtype=torch.float16, enabled=dt is torch.float16)
        for mode in ("eval", "train"):
            m.train(mode == "train")
            t.train(mode == "train")

            def hip_fwd():
                with torch.no_grad():
                    return m(x)

            def torch_fwd():
                with torch.no_grad(), cast():
                    return t(x)

            def hip_step():
                m.zero_grad(set_to_none=True)
                m(x).backward(d)

            def torch_step():
                t.zero_grad(set_to_none=True)
                with cast():
                    out = t(x)
                out.backward(d.to(out.dtype))
            if mode == "eval":
                a, b = hip_fwd(), torch_fwd().float()
                emit(f"{name}: eval-mode outputs agree to {float((a - b).norm() / b.norm()):.1e} in relative L2")
            for what, fh, ft in (("forward", hip_fwd, torch_fwd), ("forward + backward", hip_step, torch_step)):
                hip, tor = timed_pair(fh, ft, reps)
                note = "" if hip[0] <= tor[0] else "   (the HIP path is SLOWER here)"
                emit(f"  {name} {mode:5s} {what:18s} HIP {hip[0]:8.3f} ms ({hip[1]:.3f} .. {hip[2]:.3f})   torch {tor[0]:8.3f} ms ({tor[1]:.3f} .. {tor[2]:.3f})   "
                     f"torch / HIP {tor[0] / hip[0]:6.2f} x{note}")
            total, table = shares(m, x, d, 3)
            emit(f"  {name} {mode} forward + backward, profiler on: {total:.3f} ms of bracketed kernel time per step")
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
