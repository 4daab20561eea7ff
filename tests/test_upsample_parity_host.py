"""CPU-only plan checks of the nearest-x2 upsampling layers in parity form (SRGANFD_UPSAMPLE_PARITY, engine.TrunkEngine): in the 16-bit
modes each upsampling forward is one 4-class 2x2-tap launch and each data gradient one 4x4 stride-2 launch, and the backward list
holds no nearest adjoint or LeakyReLU' pass; f32 plans, and every plan with the switch at 0, keep the up=1 launches.  Library
dry-run mode: every launch goes through the C ABI's checks, no kernel runs."""
import os

import pytest
import torch


def _plan(fac, kw, dt, parity, x_shape):
    from sr_gan_fd_amd import engine as E, model as M
    old = os.environ.get("SRGANFD_UPSAMPLE_PARITY")
    os.environ["SRGANFD_UPSAMPLE_PARITY"] = "1" if parity else "0"
    try:
        net = getattr(M, fac)(**kw)
        eng = E.generator_engine(net)          # the switch is read when the engine is built
    finally:
        if old is None:
            del os.environ["SRGANFD_UPSAMPLE_PARITY"]
        else:
            os.environ["SRGANFD_UPSAMPLE_PARITY"] = old
    net.compute_dtype = dt
    x = torch.rand(*x_shape)
    sr = net(x)
    sr.sum().backward()                        # training plan: the backward list runs (dry) too
    for n, p in net.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, n
    return eng, eng._last


def _summary(eng, sp):
    """shape signature of the plan: (ksize, stride, pad, up, h_in, w_in, h_out, w_out, cin, cout, classes) per conv launch, and the C
    entry points of the backward's "call" items"""
    def sig(a):
        return (a.ksize, a.stride, a.pad, a.up, a.h_in, a.w_in, a.h_out, a.w_out, a.cin, a.cout, a.out_classes, bool(a.mask.ptr), bool(a.bias))
    fw = [sig(it.args) for it in sp.fw if it.kind == "conv"]
    bw = [sig(it.args) for it in sp.bw if it.kind == "conv"]
    calls = [it.name for it in sp.bw if it.kind == "call"]
    return fw, bw, calls


CASES = [("bsrgan_x4", dict(num_rrdb=1), (2, 3, 6, 10)),          # BSRGAN x4: two upsampling layers, ragged tiles
         ("bsrgan_x2", dict(num_rrdb=1), (1, 3, 5, 7)),           # BSRGAN x2 (builds upsampling1 unconditionally)
         ("rrdbnet_x2", dict(num_rrdb=1), (2, 3, 10, 14)),        # Real-ESRGAN x2 (PixelUnshuffle(2))
         ("rrdbnet_x1", dict(num_rrdb=1), (1, 3, 20, 12))]        # Real-ESRGAN x1 (PixelUnshuffle(4))


@pytest.mark.parametrize("fac,kw,shape", CASES)
def test_parity_plan_16bit(fac, kw, shape):
    from sr_gan_fd_amd import _abi as A
    A.set_dry_run(True)
    try:
        for dt in (torch.float16, torch.bfloat16):
            eng, sp = _plan(fac, kw, dt, True, shape)
            fw, bw, calls = _summary(eng, sp)
            n_up = eng.n_up
            assert n_up == (1 if fac == "bsrgan_x2" else 2)
            # forward: no up=1 gather left; one 4-class 2x2 launch per upsampling layer, bias + LeakyReLU, the low-res size in, 2x out
            assert not any(s[3] for s in fw)
            cls = [s for s in fw if s[10] == 4]
            assert len(cls) == n_up
            h, w = sp.H, sp.W
            for u, s in enumerate(cls):
                assert s[:2] == (2, 1) and (s[4], s[5], s[6], s[7]) == (h << u, w << u, h << u, w << u) and s[12]
            ups = [it.args for it in sp.fw if it.kind == "conv" and it.args.out_classes == 4]
            for u, a in enumerate(ups):
                assert (a.out_h_full, a.out_w_full, a.pad_y, a.pad_x, a.class_pad_step, a.act) == (sp.H << (u + 1), sp.W << (u + 1), 1, 1, 1, A.ACT_LRELU)
            # backward: one 4x4 stride-2 pad-1 launch per layer, high-res gradient in, low-res out; the mask only where the layer's input
            # is the previous upsampling conv's LeakyReLU output
            s2 = [s for s in bw if s[:3] == (4, 2, 1)]
            assert len(s2) == n_up
            assert [(s[6], s[7], s[11]) for s in s2] == [(h << (u - 1), w << (u - 1), u >= 2) for u in range(n_up, 0, -1)]
            assert not any(s[3] for s in bw)
            assert "srganfd_resample" not in calls and "srganfd_lrelu_bwd" not in calls
    finally:
        A.set_dry_run(False)


@pytest.mark.parametrize("fac,kw,shape", CASES)
def test_parity_switch_and_f32_keep_todays_plan(fac, kw, shape):
    from sr_gan_fd_amd import _abi as A
    A.set_dry_run(True)
    try:
        # f32 (parity mode of the kernels: the class launch is 16-bit only): the same plan whatever the switch says
        on = _summary(*_plan(fac, kw, torch.float32, True, shape))
        off = _summary(*_plan(fac, kw, torch.float32, False, shape))
        assert on == off
        for dt in (torch.float16, torch.bfloat16):
            eng, sp = _plan(fac, kw, dt, False, shape)
            fw, bw, calls = _summary(eng, sp)
            n_up = eng.n_up
            # switch at 0: today's launches -- the up=1 forward, the high-res data gradient, the nearest adjoints and lrelu_bwd
            assert sum(1 for s in fw if s[3]) == n_up and not any(s[10] == 4 for s in fw)
            assert not any(s[:3] == (4, 2, 1) for s in bw)
            assert calls.count("srganfd_resample") == n_up and calls.count("srganfd_lrelu_bwd") == n_up - 1
            # and the f32 plan has the same launch shapes as the 16-bit one with the switch at 0 (conv4 / conv1 differ: the thin kernels)
            assert [s for s in fw if s[8] == s[9] == 64] == [s for s in on[0] if s[8] == s[9] == 64]
    finally:
        A.set_dry_run(False)


def test_parity_packs_are_back_to_back():
    """the four class operands of each layer follow each other (what the one-launch form needs) and the 4x4 operand is separate"""
    from sr_gan_fd_amd import _abi as A, engine as E, model as M, ops
    A.set_dry_run(True)
    try:
        net = M.bsrgan_x4(num_rrdb=1)
        net.compute_dtype = torch.float16
        net(torch.rand(1, 3, 4, 4))
        eng = E.generator_engine(net)
        O = eng.packed[A.F16]["offs"]
        pb = ops.packed_bytes(A.F16, 2, 64, 64)
        for u in (1, 2):
            nm = f"upsampling{u}.0"
            assert ops.class4_ok(A.F16, 64, [O[("fc", nm, c)] for c in range(4)], pb)
            assert ("b4", nm) in O and ("f", nm) not in O and ("b", nm) not in O
    finally:
        A.set_dry_run(False)
