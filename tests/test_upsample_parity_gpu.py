"""The generator's nearest-x2 + 3x3 upsampling layers in parity form (BSRGAN/model.py:372-374; engine.TrunkEngine, SRGANFD_UPSAMPLE_PARITY):

  * forward: per output-parity class (py, px) the layer is a 2x2-tap conv over the LOW-res input whose taps are sums of the 3x3 taps
    (pack codes 14..17), all four classes in one launch (srganfd_conv_args.out_classes = 4, class_pad_step 1);
  * data gradient: conv at high res + nearest adjoint (+ LeakyReLU' of the layer below) is one 4x4 stride-2 pad-1 conv over the
    high-res gradient (pack code 18) with the mask in its epilogue.

Exactness: on inputs whose every stored 16-bit value is exact (small integers, multiples of 1/8) both paths are the same real-number
sum, so the new launches must equal the up=1 launch / the old three-pass chain bit for bit.  Random data: the new path's error against
an fp32 torch reference must stay within 2x the old path's on the same data."""
import contextlib
import copy
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

C_ = 64
SIZES = [(5, 7), (8, 8), (16, 12)]
DTYPES = [torch.float16, torch.bfloat16]


def _nhwc(t, dtype):
    return t.permute(0, 2, 3, 1).contiguous().to(dtype).cuda()


def _nchw64(t):
    return t.permute(0, 3, 1, 2).double().cpu()


def _packs(w, dt):
    """(old forward 3x3, new forward 4 classes, old data gradient 3x3, new data gradient 4x4) packed operands of the fp32 weight w"""
    from sr_gan_fd_amd import ops
    dev = torch.device("cuda")
    wc = w.cuda().float().contiguous()
    pb = ops.packed_bytes(dt, 2, C_, C_)
    cls = torch.empty(4 * pb, dtype=torch.uint8, device=dev)
    ops.PackTable([ops.pack_job(c * pb, dt, 2, C_, C_, [dict(src_off=0, co_src=C_, ci_src=C_, k_len=C_, transposed=14 + c)]) for c in range(4)],
                  dev).run(wc, cls)
    b4 = torch.empty(ops.packed_bytes(dt, 4, C_, C_), dtype=torch.uint8, device=dev)
    ops.PackTable([ops.pack_job(0, dt, 4, C_, C_, [dict(src_off=0, co_src=C_, ci_src=C_, k_len=C_, transposed=18)])], dev).run(wc, b4)
    assert ops.class4_ok(dt, C_, [c * pb for c in range(4)], pb)
    return ops.pack_single(wc, dt), cls, ops.pack_single(wc, dt, transposed=True), b4


def _fwd_old(dt, dtype, xb, packed, bias, act):
    from sr_gan_fd_amd import _abi as A, ops
    n, h, w, _ = xb.shape
    y = torch.full((n, 2 * h, 2 * w, C_), 7.0, dtype=dtype, device="cuda")
    ops.conv2d(ops.conv_args(dt, A.view(xb), A.view(y), packed, n, h, w, C_, C_, up=1, bias=bias, act=act, slope=0.2))
    torch.cuda.synchronize()
    return y


def _fwd_new(dt, dtype, xb, packed, bias, act):
    from sr_gan_fd_amd import _abi as A, ops
    n, h, w, _ = xb.shape
    y = torch.full((n, 2 * h, 2 * w, C_), 7.0, dtype=dtype, device="cuda")
    a = ops.conv_args(dt, A.view(xb), A.view(y), packed, n, h, w, C_, C_, ksize=2, stride=1, pad=0, bias=bias, act=act, slope=0.2)
    a.h_out, a.w_out = h, w
    a.out_sy, a.out_sx = 2, 2
    a.out_h_full, a.out_w_full = 2 * h, 2 * w
    a.pad_y, a.pad_x = 1, 1
    a.out_classes, a.class_pad_step = 4, 1
    ops.conv2d(a)
    torch.cuda.synchronize()
    return y


def _dgrad_old(dt, dtype, dyb, packed, maskb):
    """today's chain: the 3x3 data gradient at high res, the nearest adjoint, lrelu_bwd"""
    from sr_gan_fd_amd import _abi as A, ops
    n, H, W, _ = dyb.shape
    h, w = H // 2, W // 2
    gup = torch.full((n, H, W, C_), 7.0, dtype=dtype, device="cuda")
    ops.conv2d(ops.conv_args(dt, A.view(dyb), A.view(gup), packed, n, H, W, C_, C_))
    glo = torch.full((n, h, w, C_), 7.0, dtype=dtype, device="cuda")
    L, st = A.lib(), A.stream_ptr()
    A.check(L.srganfd_resample(0, A.view(gup), A.view(glo), dt, n, h, w, C_, st), "resample")
    if maskb is not None:
        A.check(L.srganfd_lrelu_bwd(A.view(glo), A.view(maskb), A.NULL_VIEW, A.view(glo), dt, n * h * w, C_, 0.2, st), "lrelu_bwd")
    torch.cuda.synchronize()
    return gup, glo


def _dgrad_new(dt, dtype, dyb, packed, maskb):
    from sr_gan_fd_amd import _abi as A, ops
    n, H, W, _ = dyb.shape
    glo = torch.full((n, H // 2, W // 2, C_), 7.0, dtype=dtype, device="cuda")
    ops.conv2d(ops.conv_args(dt, A.view(dyb), A.view(glo), packed, n, H, W, C_, C_, ksize=4, stride=2, pad=1,
                             mask=A.view(maskb) if maskb is not None else A.NULL_VIEW, mask_slope=0.2))
    torch.cuda.synchronize()
    return glo


def _class_taps(w):
    """the summed 2x2 class taps and 4x4 data-gradient taps of a (Co, Ci, 3, 3) weight, in float64 (what the packs hold before rounding)"""
    w = w.double()
    fsets = [[[0], [1, 2]], [[0, 1], [2]]]
    out = []
    for py in range(2):
        for px in range(2):
            for ra in fsets[py]:
                for cb in fsets[px]:
                    out.append(w[:, :, ra][:, :, :, cb].sum(dim=(2, 3)))
    bsets = [[2], [1, 2], [0, 1], [0]]
    for ru in bsets:
        for cv in bsets:
            out.append(w[:, :, ru][:, :, :, cv].sum(dim=(2, 3)))
    return torch.stack(out)


def _assert_exact_in(t, dtype, what):
    """every value a multiple of 1/8 and below 32 in magnitude: exact in bf16 (8 significant bits) and f16"""
    t = t.double()
    assert torch.equal(t * 8, torch.round(t * 8)), what
    assert t.abs().max().item() < 32, (what, t.abs().max().item())
    assert torch.equal(t.to(dtype).double(), t), what


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw", SIZES)
def test_exact_inputs_bitwise_equal_to_todays_launches(dtype, hw):
    from sr_gan_fd_amd import _abi as A, ops
    torch.manual_seed(1000 + hw[0] * 31 + hw[1])
    dt = ops.DT[dtype]
    n, (h, w) = 2, hw
    # sparse small integers (about 4 of 64 channels per pixel non-zero), weights and biases in multiples of 1/8
    x = torch.randint(-1, 2, (n, C_, h, w)).double() * (torch.rand(n, C_, h, w) < 1 / 16)
    wt = torch.randint(-2, 3, (C_, C_, 3, 3)).double() / 8
    b = torch.randint(-8, 9, (C_,)).double() / 8
    dy = torch.randint(-1, 2, (n, C_, 2 * h, 2 * w)).double() * (torch.rand(n, C_, 2 * h, 2 * w) < 1 / 16)
    act = torch.randn(n, C_, h, w)
    # the fp32 reference: every value either path stores in 16 bits is exact in the dtype
    ref_fwd = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wt, b, padding=1)
    ref_gup = F.conv_transpose2d(dy, wt, padding=1)                    # today's high-res data gradient
    ref_glo = F.avg_pool2d(ref_gup, 2) * 4                              # its nearest adjoint
    for t, what in ((x, "x"), (dy, "dy"), (ref_fwd, "conv output"), (ref_gup, "high-res gradient"), (ref_glo, "low-res gradient"),
                    (_class_taps(wt), "summed taps")):
        _assert_exact_in(t, dtype, what)
    p3, pcls, p3t, p4 = _packs(wt.float(), dt)
    bias = b.float().cuda()
    xb, dyb, mb = _nhwc(x, dtype), _nhwc(dy, dtype), _nhwc(act, dtype)
    for a_ in (A.ACT_NONE, A.ACT_LRELU):
        old, new = _fwd_old(dt, dtype, xb, p3, bias, a_), _fwd_new(dt, dtype, xb, pcls, bias, a_)
        if a_ == A.ACT_NONE:
            assert torch.equal(_nchw64(old), ref_fwd), "up=1 launch vs reference"
        # LeakyReLU: both launches run v * (v > 0 ? 1 : slope) on the same exact fp32 v (one epilogue formula): bit for bit as well
        assert torch.equal(old, new), f"forward, act {a_}: max diff {(old.float() - new.float()).abs().max().item()}"
    for mk in (None, mb):
        gup, old = _dgrad_old(dt, dtype, dyb, p3t, mk)
        new = _dgrad_new(dt, dtype, dyb, p4, mk)
        if mk is None:
            assert torch.equal(_nchw64(gup), ref_gup) and torch.equal(_nchw64(old), ref_glo), "today's chain vs reference"
        assert torch.equal(old, new), f"data gradient, mask {mk is not None}: max diff {(old.float() - new.float()).abs().max().item()}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw", SIZES)
def test_random_data_error_within_2x_of_todays(dtype, hw):
    """fp32 master weights, 16-bit-rounded activations, fp32 torch reference (float64 here).  The parity form rounds ONE sum of up to
    four taps where today's path rounds four taps: other rounding errors, the same order -- a geometry error would be orders larger."""
    from sr_gan_fd_amd import ops
    torch.manual_seed(7 + hw[0] * 31 + hw[1])
    dt = ops.DT[dtype]
    n, (h, w) = 2, hw
    x = torch.randn(n, C_, h, w).to(dtype).double()
    wt = torch.randn(C_, C_, 3, 3) * 0.06
    b = torch.randn(C_) * 0.1
    dy = torch.randn(n, C_, 2 * h, 2 * w).to(dtype).double()
    xr = x.clone().requires_grad_(True)
    ref_fwd = F.conv2d(F.interpolate(xr, scale_factor=2, mode="nearest"), wt.double(), b.double(), padding=1)
    ref_fwd.backward(dy)
    ref_dx = xr.grad
    p3, pcls, p3t, p4 = _packs(wt, dt)
    bias = b.float().cuda()
    xb, dyb = _nhwc(x, dtype), _nhwc(dy, dtype)
    from sr_gan_fd_amd import _abi as A
    e_old = (_nchw64(_fwd_old(dt, dtype, xb, p3, bias, A.ACT_NONE)) - ref_fwd.detach()).abs().max().item()
    e_new = (_nchw64(_fwd_new(dt, dtype, xb, pcls, bias, A.ACT_NONE)) - ref_fwd.detach()).abs().max().item()
    d_old = (_nchw64(_dgrad_old(dt, dtype, dyb, p3t, None)[1]) - ref_dx).abs().max().item()
    d_new = (_nchw64(_dgrad_new(dt, dtype, dyb, p4, None)) - ref_dx).abs().max().item()
    print(f"{dtype} {hw}: forward max-abs err up=1 {e_old:.3e} / parity {e_new:.3e}; data gradient today {d_old:.3e} / parity {d_new:.3e}")
    assert e_new <= 2 * e_old, (e_new, e_old)
    assert d_new <= 2 * d_old, (d_new, d_old)


@contextlib.contextmanager
def _parity(on):
    old = os.environ.get("SRGANFD_UPSAMPLE_PARITY")
    os.environ["SRGANFD_UPSAMPLE_PARITY"] = "1" if on else "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["SRGANFD_UPSAMPLE_PARITY"]
        else:
            os.environ["SRGANFD_UPSAMPLE_PARITY"] = old


def test_whole_generator_step_switch_on_and_off():
    """one f16 generator-only iteration, 23 RRDBs, batch 4, 32 -> 128, with the parity form on and off, against the f32 forward of the
    same weights.  Bounds as in the random-data test: the parity step's SR error within 2x today's; the two losses (L1 means of SR
    against one gt) then differ by at most max|SR_on - SR_off| <= err_on + err_off <= 3 err_off."""
    from sr_gan_fd_amd import engine as E, model as M
    from sr_gan_fd_amd.trainer import GeneratorTrainer
    from tests.util import scaled_init
    torch.manual_seed(0)
    g0 = M.bsrgan_x4(num_rrdb=23)
    scaled_init(g0, 3.0, 0.5)
    lr_img, gt = torch.rand(4, 3, 32, 32, device="cuda"), torch.rand(4, 3, 128, 128, device="cuda")
    ref_g = copy.deepcopy(g0).cuda()
    ref_g.compute_dtype = torch.float32
    with torch.no_grad():
        ref = ref_g(lr_img)
    out = {}
    for on in (True, False):
        g = copy.deepcopy(g0).cuda()
        g.compute_dtype = torch.float16
        with _parity(on):
            tr = GeneratorTrainer(g, lr=1e-4, betas=(0.9, 0.99), eps=1e-8, ema_decay=0.999)
        assert tr.eng.up_parity == on
        loss = tr.step(lr_img, gt)
        torch.cuda.synchronize()
        out[on] = (loss.item(), tr.sr.clone())
    err_on = (out[True][1] - ref).abs().max().item()
    err_off = (out[False][1] - ref).abs().max().item()
    dl = abs(out[True][0] - out[False][0])
    print(f"23-RRDB f16 step: SR max err vs f32 parity {err_on:.3e} / today {err_off:.3e}; loss {out[True][0]:.7f} / {out[False][0]:.7f} (diff {dl:.2e})")
    assert err_on <= 2 * err_off
    assert dl <= 3 * err_off
