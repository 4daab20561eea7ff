"""Timing + output digests of the view kernels' entry points (csrc/elementwise.hip, loss.hip, layout.hip, norm.hip's BatchNorm and the
spectral-norm gradient) at the shapes bench.py's default g_only, gan, aesrgan_gan and esrgan_gan workloads launch them with: batch 32,
f16, 128 -> 512 (aesrgan_gan 192 -> 768, esrgan_gan 32 -> 128), taken from a dry-run launch trace of two steps of each trainer
(tests/test_launch_trace_host.py's Recorder around bench.py's trainers).  One row per entry point and distinct shape; calls that differ
only in a weight or a flag that selects no other kernel share a row.  Run twice (SRGANFD_LIB=<other build>), a fresh process per run, and
compare the digests for bit-equality.  us per launch = mean of 20 launches after 3.

The shapes (npix x c in a buffer of cstride channels; n = flat fp32 elements):
  axpby            flat fp32 (c = 1, cstride 1): n = 1, 1 572 864, 4 376 900, 5 399 056, 14 499 404, 25 165 824, 56 623 104
                   f16 c = 64: npix = 32 768, 524 288, 1 179 648
  lrelu_bwd        f16, no skip: 4 718 592 x 128, 1 179 648 x 256, and channel halves of wider buffers: 18 874 368 x 64 at 64 of 128,
                   4 718 592 x 128 at 128 of 256, 1 179 648 x 256 at 256 of 512
  add_relu, gate_mul (fwd, bwd)   f16: 18 874 368 x 64 (add_relu: 4 718 592 x 64), 4 718 592 x 128 (1 179 648), 1 179 648 x 256 (294 912)
  sigmoid, sigmoid_bwd            n = 294 912, 1 179 648, 4 718 592
  l1_loss          n = 1 572 864, 25 165 824, 56 623 104 (with gradient)
  l1_loss_views    f16: 8 388 608 x 64, 18 874 368 x 64, 2 097 152 x 128, 4 718 592 x 128, 524 288 x 256, 1 179 648 x 256,
                   2 048 / 32 768 / 73 728 / 131 072 / 294 912 x 512
  l1_grad_views    f16: 2 048 x 512
  bce_logits       n = 8 388 608, 18 874 368 (loss + sigmoid mean + gradient) ; bce_logits_relativistic, sigmoid_of_mean: n = 32
  nchw_to_nhwc     f16 into a 4-channel pitch: 32 x 3 x 32^2, 128^2 (also normalised), 192^2, 512^2 (also normalised), 768^2 (also
                   normalised), 32 x 1 x 512^2, 768^2; padded to 32 channels: 32 x 3 x 128^2, 32 x 1 x 96^2, 192^2, 384^2, 1 x 1
  nhwc_to_nchw     fp32 from a 4-channel pitch, 3 channels, clamp on: 32 x 128^2, 512^2, 768^2 ; nhwc_to_nchw_scaled: 32 x 128^2
  clamp_grad_to_nhwc   f16, 4-channel pitch: 32 x 3 x 128^2, 512^2, 768^2
  batchnorm_fwd / _bwd (aesrgan_gan, y in half of a wider buffer): 18 874 368 x 64 in 128, 4 718 592 x 128 in 256, 1 179 648 x 256 in 512
  batchnorm_act_fwd / _act_bwd (esrgan_gan): 131 072 x 64, 131 072 / 32 768 x 128, 32 768 / 8 192 x 256, 8 192 / 2 048 / 512 x 512
  spectral_norm_grad   rows x cols = 64 x 576, 64 x 1152, 128 x 2304, 256 x 4608, 512 x 4096 (the discriminators launch these batched, up to
                       eight layers a call; the single-layer entry runs the same kernels with the same grids)"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sr_gan_fd_amd import _abi as A  # noqa: E402

L = A.lib()
F16, F32 = torch.float16, torch.float32
ONLY = os.environ.get("ROWS", "")            # a substring filter on the row names


def timed(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def digest(t):
    """sha1 of the bytes; past 64 MiB a position-weighted 64-bit sum of the 8-byte words, taken on the device (a multi-GB copy to the host
    and its sha1 would outlast every launch of the run)"""
    raw = t.detach().contiguous().view(-1).view(torch.uint8)
    if raw.numel() <= (1 << 26):
        return hashlib.sha1(raw.cpu().numpy().tobytes()).hexdigest()[:12]
    words = raw[:raw.numel() // 8 * 8].view(torch.int64)
    h = 0
    for lo in range(0, words.numel(), 1 << 26):
        w = words[lo:lo + (1 << 26)]
        k = torch.arange(lo, lo + w.numel(), device=w.device, dtype=torch.int64) * 2 + 1
        h = (h + int((w * k).sum().item()) + int(w.sum().item())) & 0xFFFFFFFFFFFFFFFF      # int64 products wrap: sums modulo 2^64
    return "%012x" % (h & 0xFFFFFFFFFFFF)


GEN = torch.Generator(device="cuda")


def rnd(*shape, dtype=F16, shift=0.0):
    """seeded normal values, made in slabs so that the fp32 staging of a multi-GB f16 tensor stays small"""
    out = torch.empty(shape, device="cuda", dtype=dtype)
    flat = out.view(-1)
    for lo in range(0, flat.numel(), 1 << 26):
        hi = min(lo + (1 << 26), flat.numel())
        flat[lo:hi] = (torch.randn(hi - lo, device="cuda", generator=GEN) + shift).to(dtype)
    return out


def row(name, fn, outs, once=False):
    """time fn (once: an accumulating or in-place call is digested after a single run on fresh outputs, and timed afterwards)"""
    if ONLY and ONLY not in name:
        return
    st_ = A.stream_ptr()
    if once:
        fn(st_)
        torch.cuda.synchronize()
        d = " ".join(digest(o) for o in outs)
        us = timed(lambda: fn(st_))
    else:
        us = timed(lambda: fn(st_))
        d = " ".join(digest(o) for o in outs)
    print(f"{name:44s}: {us:9.1f} us  {d}", flush=True)


def views(buf, c, c0=0):
    return A.view(buf, buf.shape[-1], c0)


def main():
    GEN.manual_seed(0)
    ws = torch.zeros(A.LOSS_WS_FLOATS, device="cuda")
    slot = torch.zeros(4, device="cuda")

    # ---- elementwise.hip
    for n in (1, 1572864, 4376900, 5399056, 14499404, 25165824, 56623104):
        x, y = rnd(n, dtype=F32), rnd(n, dtype=F32)
        row("axpby flat f32 n=%d" % n, lambda s: A.check(L.srganfd_axpby(A.View(x.data_ptr(), 1, 0), A.View(y.data_ptr(), 1, 0), A.F32, n, 1, 1.0, 1.0, s), "axpby"), [y], once=True)
        del x, y
    for npix in (32768, 524288, 1179648):
        x, y = rnd(npix, 64), rnd(npix, 64)
        row("axpby f16 %dx64" % npix, lambda s: A.check(L.srganfd_axpby(views(x, 64), views(y, 64), A.F16, npix, 64, 1.0, 1.0, s), "axpby"), [y], once=True)
        del x, y
    for npix, c, cs, c0 in ((4718592, 128, 128, 0), (1179648, 256, 256, 0), (18874368, 64, 128, 64), (4718592, 128, 256, 128), (1179648, 256, 512, 256)):
        dy, act, out = rnd(npix, cs, shift=3.0), rnd(npix, cs), torch.zeros(npix, cs, device="cuda", dtype=F16)
        row("lrelu_bwd f16 %dx%d at %d of %d" % (npix, c, c0, cs),
            lambda s: A.check(L.srganfd_lrelu_bwd(views(dy, c, c0), views(act, c, c0), A.NULL_VIEW, views(out, c, c0), A.F16, npix, c, 0.2, s), "lrelu_bwd"), [out])
        del dy, act, out
    for npix_gate, npix_add, c in ((18874368, 4718592, 64), (4718592, 1179648, 128), (1179648, 294912, 256)):
        a, b, o = rnd(npix_add, c), rnd(npix_add, c), torch.zeros(npix_add, c, device="cuda", dtype=F16)
        row("add_relu f16 %dx%d" % (npix_add, c), lambda s: A.check(L.srganfd_add_relu(views(a, c), views(b, c), views(o, c), A.F16, npix_add, c, s), "add_relu"), [o])
        del a, b, o
        x, dy, o = rnd(npix_gate, c), rnd(npix_gate, c), torch.zeros(npix_gate, c, device="cuda", dtype=F16)
        gate, dgate = torch.rand(npix_gate, device="cuda", generator=GEN), torch.zeros(npix_gate, device="cuda")
        row("gate_mul fwd f16 %dx%d" % (npix_gate, c),
            lambda s: A.check(L.srganfd_gate_mul(0, views(x, c), gate.data_ptr(), views(o, c), A.NULL_VIEW, None, A.F16, npix_gate, c, s), "gate_mul"), [o])
        row("gate_mul bwd f16 %dx%d" % (npix_gate, c),
            lambda s: A.check(L.srganfd_gate_mul(1, views(x, c), gate.data_ptr(), views(dy, c), views(o, c), dgate.data_ptr(), A.F16, npix_gate, c, s), "gate_mul"), [o, dgate])
        del x, dy, o, gate, dgate
    for n in (294912, 1179648, 4718592):
        x, ds, o = rnd(n, dtype=F32), rnd(n, dtype=F32), torch.zeros(n, device="cuda")
        row("sigmoid n=%d" % n, lambda s: A.check(L.srganfd_sigmoid(x.data_ptr(), n, s), "sigmoid"), [x], once=True)
        row("sigmoid_bwd n=%d" % n, lambda s: A.check(L.srganfd_sigmoid_bwd(ds.data_ptr(), x.data_ptr(), o.data_ptr(), n, s), "sigmoid_bwd"), [o])

    # ---- loss.hip
    for n in (1572864, 25165824, 56623104):
        a, b, g = rnd(n, dtype=F32), rnd(n, dtype=F32), torch.zeros(n, device="cuda")
        row("l1_loss n=%d" % n, lambda s: A.check(L.srganfd_l1_loss(a.data_ptr(), b.data_ptr(), n, 20.0, slot.data_ptr(), 0, g.data_ptr(), 20.0, None, ws.data_ptr(), s), "l1"), [slot, g])
        del a, b, g
    for npix, c in ((8388608, 64), (18874368, 64), (2097152, 128), (4718592, 128), (524288, 256), (1179648, 256), (2048, 512), (32768, 512), (73728, 512),
                    (131072, 512), (294912, 512)):
        a, b = rnd(npix, c), rnd(npix, c)
        row("l1_loss_views f16 %dx%d" % (npix, c),
            lambda s: A.check(L.srganfd_l1_loss_views(views(a, c), views(b, c), A.F16, npix, c, 0, 1.0, slot.data_ptr(), 0, ws.data_ptr(), s), "l1_views"), [slot])
        del a, b
    a, b, o, up = rnd(2048, 512), rnd(2048, 512), torch.zeros(2048, 512, device="cuda", dtype=F16), torch.full((1,), 1024.0, device="cuda")
    row("l1_grad_views f16 2048x512", lambda s: A.check(L.srganfd_l1_grad_views(views(a, 512), views(b, 512), views(o, 512), A.F16, 2048, 512, up.data_ptr(), 9.54e-07, s), "l1_grad"), [o])
    for n in (8388608, 18874368):
        x, g, sig = rnd(n, dtype=F32), torch.zeros(n, device="cuda"), torch.zeros(1, device="cuda")
        row("bce_logits n=%d" % n, lambda s: A.check(L.srganfd_bce_logits(x.data_ptr(), n, 1.0, 1.0, slot.data_ptr(), 0, sig.data_ptr(), g.data_ptr(), 1.0, None, ws.data_ptr(), s), "bce"), [slot, sig, g])
        del x, g
    x, other, gx, go = rnd(32, dtype=F32), rnd(32, dtype=F32), torch.zeros(32, device="cuda"), torch.zeros(32, device="cuda")
    row("bce_logits_relativistic n=32", lambda s: A.check(L.srganfd_bce_logits_relativistic(x.data_ptr(), 32, other.data_ptr(), 32, 1.0, 0.5, slot.data_ptr(), 0, gx.data_ptr(), 0,
                                                                                           go.data_ptr(), 0, 0.5, None, ws.data_ptr(), s), "bce_rel"), [slot, gx, go])
    row("sigmoid_of_mean n=32", lambda s: A.check(L.srganfd_sigmoid_of_mean(x.data_ptr(), 32, slot.data_ptr(), ws.data_ptr(), s), "sigmoid_of_mean"), [slot])

    # ---- layout.hip
    mean, std = torch.tensor([0.485, 0.456, 0.406], device="cuda"), torch.tensor([0.229, 0.224, 0.225], device="cuda")
    for c, h, cpad, norm in ((3, 32, 4, False), (3, 128, 4, False), (3, 128, 4, True), (3, 192, 4, False), (3, 512, 4, False), (3, 512, 4, True), (3, 768, 4, False), (3, 768, 4, True),
                             (1, 512, 4, False), (1, 768, 4, False), (3, 128, 32, False), (1, 96, 32, False), (1, 192, 32, False), (1, 384, 32, False), (1, 1, 32, False)):
        src, dst = rnd(32, c, h, h, dtype=F32), torch.zeros(32, h, h, cpad, device="cuda", dtype=F16)
        row("nchw_to_nhwc f16 32x%dx%d^2 to %d%s" % (c, h, cpad, " normalised" if norm else ""),
            lambda s: A.check(L.srganfd_nchw_to_nhwc(src.data_ptr(), 32, c, h, h, views(dst, cpad), A.F16, cpad, mean.data_ptr() if norm else None, std.data_ptr() if norm else None, s), "nchw_to_nhwc"), [dst])
        del src, dst
    for h in (128, 512, 768):
        src, dst = rnd(32, h, h, 4, dtype=F32), torch.zeros(32, 3, h, h, device="cuda")
        row("nhwc_to_nchw f32 32x3x%d^2 clamp" % h, lambda s: A.check(L.srganfd_nhwc_to_nchw(views(src, 3), A.F32, 32, 3, h, h, dst.data_ptr(), 1, s), "nhwc_to_nchw"), [dst])
        if h == 128:
            row("nhwc_to_nchw_scaled 32x3x128^2", lambda s: A.check(L.srganfd_nhwc_to_nchw_scaled(views(src, 3), 32, 3, h, h, dst.data_ptr(), std.data_ptr(), s), "nhwc_to_nchw_scaled"), [dst])
        dsr, g = rnd(32, 3, h, h, dtype=F32), torch.zeros(32, h, h, 4, device="cuda", dtype=F16)
        row("clamp_grad_to_nhwc f16 32x3x%d^2" % h, lambda s: A.check(L.srganfd_clamp_grad_to_nhwc(dsr.data_ptr(), views(src, 4), 32, 3, h, h, views(g, 4), A.F16, 4, s), "clamp_grad"), [g])
        del src, dst, dsr, g

    # ---- norm.hip: BatchNorm (training mode), the spectral-norm gradient
    def bn(npix, c, cs_y, act):
        x, y = rnd(npix, c), torch.zeros(npix, cs_y, device="cuda", dtype=F16)
        dy, dx = rnd(npix, cs_y), torch.zeros(npix, c, device="cuda", dtype=F16)
        gamma, beta = torch.rand(c, device="cuda", generator=GEN) + 0.5, rnd(c, dtype=F32)
        rm, rv, save = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda"), torch.zeros(4 * c, device="cuda")
        dgamma, dbeta = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
        bws = torch.zeros(L.srganfd_batchnorm_partial_floats(c) + 3 * c, device="cuda")
        tag = "f16 %dx%d in %d" % (npix, c, cs_y)
        if act:
            row("batchnorm_act_fwd " + tag, lambda s: A.check(L.srganfd_batchnorm_act_fwd(views(x, c), views(y, c), A.F16, npix, c, gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(),
                                                                                           0.1, 1e-5, 1, save.data_ptr(), bws.data_ptr(), 0.2, s), "bn"), [y, save, rm, rv], once=True)
            row("batchnorm_act_bwd " + tag, lambda s: A.check(L.srganfd_batchnorm_act_bwd(views(x, c), views(dy, c), views(dx, c), A.F16, npix, c, gamma.data_ptr(), save.data_ptr(), dgamma.data_ptr(),
                                                                                           dbeta.data_ptr(), 0.0, bws.data_ptr(), views(y, c), 0.2, s), "bn"), [dx, dgamma, dbeta])
        else:
            row("batchnorm_fwd " + tag, lambda s: A.check(L.srganfd_batchnorm_fwd(views(x, c), views(y, c), A.F16, npix, c, gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), 0.1, 1e-5, 1,
                                                                                   save.data_ptr(), bws.data_ptr(), s), "bn"), [y, save, rm, rv], once=True)
            row("batchnorm_bwd " + tag, lambda s: A.check(L.srganfd_batchnorm_bwd(views(x, c), views(dy, c), views(dx, c), A.F16, npix, c, gamma.data_ptr(), save.data_ptr(), dgamma.data_ptr(),
                                                                                   dbeta.data_ptr(), 0.0, bws.data_ptr(), s), "bn"), [dx, dgamma, dbeta])

    for npix, c in ((18874368, 64), (4718592, 128), (1179648, 256)):
        bn(npix, c, 2 * c, False)
    for npix, c in ((131072, 64), (131072, 128), (32768, 128), (32768, 256), (8192, 256), (8192, 512), (2048, 512), (512, 512)):
        bn(npix, c, c, True)
    for rows, cols in ((64, 576), (64, 1152), (128, 2304), (256, 4608), (512, 4096)):
        G, W, dW = rnd(rows, cols, dtype=F32), rnd(rows, cols, dtype=F32), torch.zeros(rows, cols, device="cuda")
        u, v, inv = rnd(rows, dtype=F32), rnd(cols, dtype=F32), torch.full((1,), 0.37, device="cuda")
        sws = torch.zeros(1025, device="cuda")
        row("spectral_norm_grad %dx%d" % (rows, cols), lambda s: A.check(L.srganfd_spectral_norm_grad(G.data_ptr(), W.data_ptr(), u.data_ptr(), v.data_ptr(), inv.data_ptr(), dW.data_ptr(), rows, cols, 0.0,
                                                                                                    sws.data_ptr(), s), "sn_grad"), [dW])


if __name__ == "__main__":
    main()
