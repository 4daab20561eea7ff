"""tests/norm_oracle.py against torch's own float64 operators under autograd (no GPU): what makes the comparisons of
tests/test_norm_gpu.py and tests/test_attention_gate_gpu.py trustworthy.  Also the argument checks of the BatchNorm entry points, in the
library's dry-run mode (validates, launches nothing)."""
import pytest
import torch
import torch.nn.functional as F

from tests import norm_oracle as O

RTOL = 1e-12


def _close(got, want, what):
    want = want.detach().double()
    e = ((got.double() - want).abs().max() / (want.abs().max() + 1e-300)).item()
    assert e <= RTOL, f"{what}: {e:.3e}"


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _bn_case(c, seed, zero_channel=False):
    g = torch.Generator().manual_seed(seed)
    n, h, w = 2, 7, 15                                                  # 210 pixels: no power of two anywhere
    ch = torch.arange(c, dtype=torch.float64)
    x = torch.randn(n, h, w, c, generator=g, dtype=torch.float64) * (0.5 + (ch % 7) / 6) + torch.sin(ch) * 1.5
    gamma, beta = 0.5 + (ch % 5) / 4, torch.cos(ch * 0.7)
    if zero_channel:
        gamma[c // 2] = beta[c // 2] = 0.0
    rm, rv = torch.randn(c, generator=g, dtype=torch.float64), torch.rand(c, generator=g, dtype=torch.float64) + 0.5
    dy = torch.randn(n, h, w, c, generator=g, dtype=torch.float64)
    return x, gamma, beta, rm, rv, dy


@pytest.mark.parametrize("c", [8, 64, 264])
@pytest.mark.parametrize("slope", [1.0, 0.2])
def test_batchnorm_training_forward_and_backward_equal_torch_float64(c, slope):
    x, gamma, beta, rm, rv, dy = _bn_case(c, 10 + c, zero_channel=slope != 1.0)
    xt, gt, bt = _nchw(x).clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    trm, trv = rm.clone(), rv.clone()
    yt = F.leaky_relu(F.batch_norm(xt, trm, trv, gt, bt, True, 0.1, 1e-5), slope)
    yt.backward(_nchw(dy))
    y, rm2, rv2, save = O.bn_forward(x, gamma, beta, rm, rv, 0.1, 1e-5, True, slope)
    _close(_nchw(y), yt, "y")
    _close(rm2, trm, "running_mean")
    _close(rv2, trv, "running_var")
    xf = x.reshape(-1, c)
    _close(save[:c], xf.mean(0), "save.mean")
    _close(save[c:2 * c], (xf.var(0, unbiased=False) + 1e-5).rsqrt(), "save.invstd")
    _close(save[2 * c:3 * c], gamma * save[c:2 * c], "save.scale")
    _close(save[3 * c:], beta - save[:c] * save[2 * c:3 * c], "save.shift")
    if slope != 1.0:
        assert (y[..., c // 2] == 0).all()                              # the gamma = beta = 0 channel: LeakyReLU'(0) is the slope below
    dx, dgamma, dbeta = O.bn_backward(x, dy, gamma, save, act=y if slope != 1.0 else None, slope=slope)
    _close(_nchw(dx), xt.grad, "dx")
    _close(dgamma, gt.grad, "dgamma")
    _close(dbeta, bt.grad, "dbeta")


def test_batchnorm_eval_mode_uses_and_keeps_the_running_statistics():
    c = 24
    x, gamma, beta, rm, rv, _ = _bn_case(c, 3)
    y, rm2, rv2, save = O.bn_forward(x, gamma, beta, rm, rv, 0.1, 1e-5, False, 0.2)
    _close(_nchw(y), F.leaky_relu(F.batch_norm(_nchw(x), rm.clone(), rv.clone(), gamma, beta, False, 0.1, 1e-5), 0.2), "y")
    assert torch.equal(rm2, rm) and torch.equal(rv2, rv)
    _close(save[:c], rm, "save.mean")
    _close(save[c:2 * c], (rv + 1e-5).rsqrt(), "save.invstd")


def test_batchnorm_one_value_per_channel_is_refused_like_torch():
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        F.batch_norm(torch.zeros(1, 8, 1, 1), torch.zeros(8), torch.ones(8), None, None, True)
    with pytest.raises(ValueError, match="more than one value"):
        O.bn_forward(torch.zeros(1, 1, 1, 8), torch.ones(8), torch.zeros(8), torch.zeros(8), torch.ones(8), 0.1, 1e-5, True)


def test_batchnorm_backward_of_a_share_with_global_sums_is_the_full_batch_slice():
    c = 16
    x, gamma, beta, rm, rv, dy = _bn_case(c, 5)
    x, dy = torch.cat([x, x.flip(1) * 1.5]), torch.cat([dy, dy.flip(2)])          # 4 images: 3 + 1
    _, _, _, save = O.bn_forward(x, gamma, beta, rm, rv, 0.1, 1e-5, True)
    dx, dgamma, dbeta = O.bn_backward(x, dy, gamma, save)
    parts = [O.bn_backward(x[a:b], dy[a:b], gamma, save, total=x.numel() // c, global_sums=(dbeta, dgamma)) for a, b in ((0, 3), (3, 4))]
    _close(torch.cat([p[0] for p in parts]), dx, "dx")
    _close(parts[0][1] + parts[1][1], dgamma, "dgamma")
    _close(parts[0][2] + parts[1][2], dbeta, "dbeta")
    assert (parts[1][1] - dgamma).abs().max() > 1e-3                               # a share's own sums are not the batch's


@pytest.mark.parametrize("sizes", O.RESIZE_PAIRS, ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_resize_bilinear_equals_interpolate_and_its_adjoint(sizes):
    (hi, wi), (ho, wo) = sizes
    g = torch.Generator().manual_seed(hi * 1000 + wo)
    x = torch.randn(2, hi, wi, 8, generator=g, dtype=torch.float64)
    dy = torch.randn(2, ho, wo, 8, generator=g, dtype=torch.float64)
    xt = _nchw(x).clone().requires_grad_(True)
    yt = F.interpolate(xt, size=(ho, wo), mode="bilinear", align_corners=False)
    yt.backward(_nchw(dy))
    y, dx = O.resize_bilinear(x, ho, wo), O.resize_bilinear_backward(dy, hi, wi)
    assert y.shape == (2, ho, wo, 8) and dx.shape == x.shape
    _close(_nchw(y), yt, "y")
    _close(_nchw(dx), xt.grad, "dx")
    lhs, rhs = (y * dy).sum().item(), (x * dx).sum().item()
    assert abs(lhs - rhs) <= RTOL * max(abs(lhs), (y * dy).abs().sum().item())
    assert torch.allclose(O.resize_matrix(hi, ho).sum(1), torch.ones(ho, dtype=torch.float64), rtol=0, atol=1e-15)


def test_add_relu_and_gate_equal_autograd():
    g = torch.Generator().manual_seed(7)
    a, b = torch.randn(3, 5, 7, 8, generator=g, dtype=torch.float64), torch.randn(3, 5, 7, 8, generator=g, dtype=torch.float64)
    b[0, 0, 0] = -a[0, 0, 0]
    r = O.add_relu(a, b)
    assert torch.equal(r, F.relu(a + b)) and (r[0, 0, 0] == 0).all() and not torch.signbit(r[0, 0, 0]).any()
    x = a.clone().requires_grad_(True)
    gt = torch.rand(3, 5, 7, generator=g, dtype=torch.float64).requires_grad_(True)
    yt = gt.unsqueeze(-1) * x
    yt.backward(b)
    _close(O.gate(a, gt), yt, "gate")
    dx, dgate = O.gate_backward(a, gt, b)
    _close(dx, x.grad, "dx")
    _close(dgate, gt.grad, "dgate")


def test_maxpool_and_its_backward_through_relu_equal_autograd_with_ties():
    g = torch.Generator().manual_seed(9)
    z = torch.round(torch.randn(2, 6, 10, 5, generator=g, dtype=torch.float64) * 2) / 2      # a coarse grid: many ties
    z[0, 0:2, 0:2] = -1.0                                                                      # a window with nothing positive
    z[0, 2:4, 2:4] = 0.75                                                                      # four equal maxima
    z[1, 0, 0], z[1, 0, 1], z[1, 1, 0], z[1, 1, 1] = 0.5, 2.0, 2.0, 2.0                         # the first of three
    zt = _nchw(z).clone().requires_grad_(True)
    yt = F.max_pool2d(F.relu(zt), 2, 2)
    dy = torch.randn(2, 3, 5, 5, generator=g, dtype=torch.float64)
    yt.backward(_nchw(dy))
    x = F.relu(z)
    assert torch.equal(_nchw(O.maxpool2(x)), yt.detach())
    dx = O.maxpool2_relu_backward(x, dy)
    assert torch.equal(_nchw(dx), zt.grad)
    assert (dx[0, 0:2, 0:2] == 0).all() and (dx[0, 2, 2] == dy[0, 1, 1]).all() and (dx[0, 2:4, 2:4].sum((0, 1)) == dy[0, 1, 1]).all()
    assert (dx[1, 0, 1] == dy[1, 0, 0]).all()


def test_ulp_and_the_stored_bound():
    r = torch.tensor([1.0, 1.5, 1.999, 2.0, 0.75, 0.0, -3.0, 1e-6], dtype=torch.float64)
    want = torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 0.0, 2.0 ** -6, 2.0 ** -27], dtype=torch.float64)
    assert torch.equal(O.ulp(r, torch.bfloat16), want)
    assert torch.equal(O.ulp(r, torch.float16), want / 8)
    for dt in (torch.bfloat16, torch.float16):
        ref = torch.randn(4096, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
        O.assert_stored(ref.to(dt), ref, 0.0, "correctly rounded")
        off = (ref + 2.5 * O.ulp(ref, dt)).to(dt)
        with pytest.raises(AssertionError):
            O.assert_stored(off, ref, 0.0, "two ulps off")
    with pytest.raises(AssertionError):
        O.assert_f32(torch.tensor([1.0, 2.0 + 1e-4]), torch.tensor([1.0, 2.0]), 1e-5, "fp32")


def test_batchnorm_entry_points_refuse_bad_shapes_before_launching():
    from sr_gan_fd_amd import _abi as A
    L = A.lib()
    A.set_dry_run(True)
    try:
        p = 4096                                              # a non-null, 16-byte aligned address; nothing is dereferenced in dry-run mode
        err = lambda: L.srganfd_last_error().decode()
        V = lambda c, c0=0: A.View(p, c + 32, c0, 0, 0)

        def fwd(dt, npix, c, training=1, c0=0):
            return L.srganfd_batchnorm_fwd(V(c, c0), V(c), dt, npix, c, p, p, p, p, 0.1, 1e-5, training, p, p, 0)

        def bwd(dt, npix, c, c0=0):
            return L.srganfd_batchnorm_act_bwd(V(c), V(c, c0), V(c), dt, npix, c, p, p, p, p, 0.0, p, V(c), 0.2, 0)

        for dt, c in ((A.F32, 8), (A.BF16, 8), (A.F16, 264), (A.F32, 264), (A.F16, 384), (A.F32, 512)):
            assert fwd(dt, 210, c) == 0 and bwd(dt, 210, c) == 0, err()
        for dt, c, cc in ((A.BF16, 280, 24), (A.F16, 280, 24), (A.F32, 268, 12)):
            assert fwd(dt, 210, c) == -1 and f"channel block of {cc}" in err()
            assert bwd(dt, 210, c) == -1 and f"channel block of {cc}" in err()
        assert fwd(A.F16, 210, 4) == -1 and bwd(A.BF16, 210, 4) == -1 and fwd(A.F32, 210, 6) == -1
        assert fwd(A.F16, 210, 64, c0=4) == -1 and bwd(A.F32, 210, 64, c0=2) == -1
        assert fwd(A.F32, 1, 64) == -1 and "more than one value per channel" in err()
        assert fwd(A.F32, 0, 64) == -1
        assert fwd(A.F32, 1, 64, training=0) == 0 and fwd(A.F32, 2, 64) == 0
        sync = lambda phase, npix, total, c=64: L.srganfd_batchnorm_fwd_sync(V(c), V(c), A.BF16, npix, c, p, p, p, p, 0.1, 1e-5, p, p, 0.2, phase, total, 0)
        assert sync(1, 1, 0) == 0 and sync(2, 1, 4) == 0               # a rank may hold one pixel of a larger batch
        assert sync(2, 1, 1) == -1 and "more than one value per channel" in err()
        assert sync(1, 210, 0, c=264) == -1 and sync(2, 210, 420, c=264) == -1 and "at most 256 channels" in err()
        assert L.srganfd_batchnorm_bwd_sync(V(264), V(264), V(264), A.F16, 210, 264, p, p, p, p, 0.0, p, p, A.NULL_VIEW, 1.0, 1, 0, 0) == -1
    finally:
        A.set_dry_run(False)
