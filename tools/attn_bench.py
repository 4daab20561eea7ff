"""Times model.SelfAttention (fused HIP attention between two 1x1-conv projections) beside torch's nn.MultiheadAttention called as
the reference calls it (BSRGAN/model.py:395-402: need_weights on, the unfused path), on the same GPU, weights and inputs:
warm-up, device events around each call, median of the repetitions.
    python tools/attn_bench.py [--reps 30] [--out profiles/attention_bench.txt]
Shapes: the consumers' -- batch 16 of 36 x 36 tokens at 256 channels / 8 heads and of 18 x 18 at 512 / 8 (the U-Net
discriminator's two attention layers at a 144 x 144 crop), and 3600 sequences of 8 tokens at 64 / 4 (the transformer generator, which
attends over the batch index).  Rows: forward without the weights result, forward with it, backward alone (of the forward with
weights).  Precisions: fp32, and float16 (the HIP module pinned to it, torch under autocast)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sr_gan_fd_amd import model as M  # noqa: E402

SHAPES = ((16, 256, 36, 36, 8), (16, 512, 18, 18, 8), (3600, 64, 2, 4, 4))


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


def reference_forward(mha, x, need_weights=True):
    """SelfAttention.forward of the reference over torch's module"""
    b, c, h, w = x.shape
    t = x.view(b, c, -1).permute(2, 0, 1)
    out, weights = mha(t, t, t, need_weights=need_weights)
    return out.permute(1, 2, 0).reshape(b, c, h, w), weights


def rows(reps):
    dev = torch.device("cuda", 0)
    lines = [f"device: {torch.cuda.get_device_name(0)}; median (min .. max) of {reps} calls, device events, 5 warm-up calls",
             "HIP: model.SelfAttention (nchw_to_nhwc, 1x1 conv, attention_fwd [, attention_weights], 1x1 conv, nhwc_to_nchw; backward alike)",
             "torch: nn.MultiheadAttention(x, x, x) on the permuted view, need_weights on as the reference calls it (its unfused path)"]
    for b, c, h, w, heads in SHAPES:
        for name, dt in (("fp32", torch.float32), ("f16", torch.float16)):
            torch.manual_seed(0)
            m = M.SelfAttention(c, heads).to(dev)
            m.compute_dtype = dt
            mha = torch.nn.MultiheadAttention(c, heads).to(dev)
            mha.load_state_dict(m.multihead_attention.state_dict())
            x = torch.randn(b, c, h, w, device=dev, requires_grad=True)
            d = torch.randn(b, c, h, w, device=dev)
            cast = torch.autocast("cuda", dtype=torch.float16, enabled=dt is torch.float16)

            def hip_fwd(weights):
                m.need_weights = weights
                with torch.no_grad():
                    return m(x)

            def torch_fwd(weights):
                with torch.no_grad(), cast:
                    return reference_forward(mha, x, weights)
            a, t = hip_fwd(True), torch_fwd(True)
            diff = [float((p.float() - q.float()).abs().max() / q.float().abs().max()) for p, q in zip(a, t)]
            lines.append(f"batch {b}, {h} x {w} tokens, {c} channels / {heads} heads, {name}: HIP and torch agree to {diff[0]:.1e} (output) / {diff[1]:.1e} (weights) of the maximum")
            def hip_bwd():
                # (the module keeps one set of activations: the backward timed here belongs to the forward just before it)
                m.need_weights = True
                out = m(x)[0]
                return lambda: out.backward(d, retain_graph=True)

            def torch_bwd():
                with cast:
                    out = reference_forward(mha, x)[0]
                return lambda: out.backward(d.to(out.dtype), retain_graph=True)
            table = (("forward", lambda: (lambda: hip_fwd(False)), lambda: (lambda: torch_fwd(False))),
                     ("forward + weights", lambda: (lambda: hip_fwd(True)), lambda: (lambda: torch_fwd(True))),
                     ("backward", hip_bwd, torch_bwd))
            for what, f_hip, f_torch in table:
                hip, tor = median_ms(f_hip(), reps), median_ms(f_torch(), reps)
                note = "" if hip[0] <= tor[0] else "   (the HIP path is SLOWER here)"
                lines.append(f"  {what:18s} HIP {hip[0]:8.3f} ms ({hip[1]:.3f} .. {hip[2]:.3f})   torch {tor[0]:8.3f} ms ({tor[1]:.3f} .. {tor[2]:.3f})   "
                             f"torch / HIP {tor[0] / hip[0]:6.2f} x{note}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    text = "\n".join(rows(args.reps))
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
