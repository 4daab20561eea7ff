#!/usr/bin/env python3
"""bsrgantrans_x2 at A-ESRGAN's training shape -- batch 8, LR 60 x 60, 23 RRDBs: 900 sequences of 8 tokens -- on one GPU:

  * forward and forward + backward of the module, f16 and fp32, eval and train (p = 0.1), against a torch restatement of the same
    network (own text below: F.conv2d and torch's nn.TransformerEncoder, autocast for f16) with the same state dict on the same GPU,
    and against this project's bsrgan_x2 at the same shape (the stage's added cost);
  * the share of the stage's launches in the generator's forward and backward lists (device events around every item of the lists);
  * one fused GeneratorTrainer step, eager and as a captured graph (is the step launch-bound outside a graph?).
Alternating runs, medians, device events.  No speed is a pass condition; fp32 is reported as measured.

    python tools/bsrgantrans_bench.py [--rounds 7] [--out profiles/bsrgantrans_bench.txt]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sr_gan_fd_amd import model as M, ops  # noqa: E402
from sr_gan_fd_amd.engine import generator_engine  # noqa: E402
from sr_gan_fd_amd.graph import GraphedStep  # noqa: E402
from sr_gan_fd_amd.trainer import GeneratorTrainer  # noqa: E402

DEV = torch.device("cuda", 0)
B, H, W, RRDB = 8, 60, 60, 23


class TorchBSRGANtrans(torch.nn.Module):
    """the same function in torch ops, parameters under the same state-dict keys"""

    def __init__(self, ours):
        super().__init__()
        self.P = torch.nn.ParameterDict({k.replace(".", "/"): torch.nn.Parameter(v.detach().clone()) for k, v in ours.named_parameters()
                                         if not k.startswith("transformer_")})
        self.enc = torch.nn.TransformerEncoder(torch.nn.TransformerEncoderLayer(64, 4), 2, enable_nested_tensor=False)
        self.enc.load_state_dict(ours.transformer_encoder.state_dict())
        self.n = len(ours.trunk)

    def conv(self, x, name, stride=1):
        return F.conv2d(x, self.P[name.replace(".", "/") + "/weight"], self.P[name.replace(".", "/") + "/bias"], stride=stride, padding=1)

    def forward(self, x):
        lre = lambda t: F.leaky_relu(t, 0.2)
        up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")
        out1 = cur = self.conv(x, "conv1")
        for i in range(self.n):
            x0 = cur
            for r in (1, 2, 3):
                feats = [cur]
                for k in range(1, 5):
                    feats.append(lre(self.conv(torch.cat(feats, 1), "trunk.%d.rdb%d.conv%d" % (i, r, k))))
                cur = self.conv(torch.cat(feats, 1), "trunk.%d.rdb%d.conv5" % (i, r)) * 0.2 + cur
            cur = cur * 0.2 + x0
        t = lre(self.conv(cur, "downsamplingTrans.0", 2))
        b, c, h, w = t.shape
        t = self.enc(t.permute(0, 2, 3, 1).flatten(1, 2)).view(b, h, w, c).permute(0, 3, 1, 2)
        t = lre(self.conv(up(t), "upsamplingTrans.0"))
        t = self.conv(t, "conv2") + out1
        t = lre(self.conv(up(t), "upsampling1.0"))
        return torch.clamp(self.conv(lre(self.conv(t, "conv3.0")), "conv4"), 0.0, 1.0)


def timed(fn, rounds):
    """median milliseconds of fn() per candidate, the candidates alternating inside every round"""
    ts = {k: [] for k in fn}
    for k in fn:
        fn[k]()
        fn[k]()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, f in fn.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b))
    return {k: statistics.median(v) for k, v in ts.items()}


def per_item(items, run):
    out = []
    for it in items:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        it.launch(run)
        b.record()
        b.synchronize()
        out.append((getattr(it, "label", None) or it.kind, a.elapsed_time(b)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []
    say = lambda s: (print(s, flush=True), lines.append(s))
    torch.manual_seed(0)
    ours = M.bsrgantrans_x2(num_rrdb=RRDB).to(DEV)
    plain = M.bsrgan_x2(num_rrdb=RRDB).to(DEV)
    ref = TorchBSRGANtrans(ours).to(DEV)
    x = torch.rand(B, 3, H, W, device=DEV)
    d = torch.randn(B, 3, 2 * H, 2 * W, device=DEV)
    say("bsrgantrans_x2, batch %d, LR %d x %d, %d RRDBs, %s; medians of %d alternating rounds, ms" % (B, H, W, RRDB, torch.cuda.get_device_name(0), args.rounds))
    for dt in (torch.float16, torch.float32):
        for mode in ("eval", "train"):
            for m in (ours, plain, ref):
                m.train(mode == "train")
            ours.compute_dtype = plain.compute_dtype = dt

            def fwd(m, torch_path=False):
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=torch_path and dt == torch.float16):
                    return m(x)

            def fb(m, torch_path=False):
                for p in m.parameters():
                    p.grad = None
                with torch.autocast("cuda", dtype=torch.float16, enabled=torch_path and dt == torch.float16):
                    y = m(x)
                y.backward(d)
            f = timed({"hip": lambda: fwd(ours), "torch": lambda: fwd(ref, True), "bsrgan_x2": lambda: fwd(plain)}, args.rounds)
            g = timed({"hip": lambda: fb(ours), "torch": lambda: fb(ref, True), "bsrgan_x2": lambda: fb(plain)}, args.rounds)
            say("%-4s %-5s forward            hip %7.2f   torch %7.2f (x%.2f)   bsrgan_x2 %7.2f (the stage adds %.2f)" %
                (str(dt)[6:], mode, f["hip"], f["torch"], f["torch"] / f["hip"], f["bsrgan_x2"], f["hip"] - f["bsrgan_x2"]))
            say("%-4s %-5s forward + backward hip %7.2f   torch %7.2f (x%.2f)   bsrgan_x2 %7.2f (the stage adds %.2f)" %
                (str(dt)[6:], mode, g["hip"], g["torch"], g["torch"] / g["hip"], g["bsrgan_x2"], g["hip"] - g["bsrgan_x2"]))
    # the stage's launches, item by item (f16, train): every item between two events, so launch gaps are inside each figure
    ours.train()
    ours.compute_dtype = torch.float16
    eng = generator_engine(ours)
    y = ours(x.clone().requires_grad_(True))
    sp = eng._last
    grad = eng.fp.new_grad(DEV)
    marks = [i for i, it in enumerate(sp.bw) if it.kind == "ready"]          # the stage's backward: between the first two bucket markers
    for name, items, run in (("forward", sp.fw, ops.Run("conv2d", training=True)),
                             ("backward", sp.bw, ops.Run("conv2d(dgrad)", grad=grad.data_ptr(), ws=sp.wg_ws))):
        rows = per_item(items, run)
        rows = per_item(items, run)
        total = sum(t for _, t in rows)
        if name == "forward":
            first = next(i for i, it in enumerate(items) if it.kind == "conv" and it.args.stride == 2 and it.args.ksize == 3)
            stage = rows[first:first + 1 + sp.t_len[0] + 1] + rows[:1]
        else:
            stage = rows[marks[0] + 1:marks[1]]
        say("f16 train %s list: %d items %.2f ms item by item; the stage's %d items %.2f ms (%.1f %%)" %
            (name, len(rows), total, len(stage), sum(t for _, t in stage), 100 * sum(t for _, t in stage) / total))
        agg = {}
        for label, t in stage:
            agg[label] = agg.get(label, 0.0) + t
        for label, t in sorted(agg.items(), key=lambda kv: -kv[1]):
            say("    %-60s %.3f ms (%.1f %% of the stage)" % (label, t, 100 * t / sum(agg.values())))
    y.sum().backward()
    # the fused step, eager and graphed
    gt = torch.rand(B, 3, 2 * H, 2 * W, device=DEV)
    tr = GeneratorTrainer(ours, lr=1e-4, betas=(0.9, 0.99), eps=1e-4)
    graphed = GraphedStep(tr, x, gt, warmup=2)
    tr2 = GeneratorTrainer(M.bsrgantrans_x2(num_rrdb=RRDB).to(DEV).train(), lr=1e-4, betas=(0.9, 0.99), eps=1e-4)
    s = timed({"eager": lambda: tr2.step(x, gt), "graphed": lambda: graphed(x, gt)}, args.rounds)
    say("f16 GeneratorTrainer step (train mode, p = 0.1): eager %.2f ms, graphed %.2f ms -> %s outside a graph" %
        (s["eager"], s["graphed"], "launch-bound" if s["eager"] > 1.15 * s["graphed"] else "not launch-bound"))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
