"""The kernels of the A-ESRGAN attention gates (general bilinear resize and its adjoint, relu(a + b), the gate multiply and its
backward with the per-pixel channel reduction) and the 2x2 max-pool pair of the VGG tap, each on its own against the float64
definitions of tests/norm_oracle.py: every dtype, channel-slice views with sentinels around them, every width of the shuffle reduction.

Bounds as in tests/test_norm_gpu.py: fp32 within 1e-5 (forward) / 1e-4 (backward) of float64 relative to max|ref|, a stored 16-bit
result within one ulp of its type on top of that; max-pool and its backward bit for bit."""
import pytest
import torch

from tests import norm_oracle as O

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]
SENTINEL, Slot = O.SENTINEL, O.Slot


def _vn(dtype):
    return 4 if dtype == torch.float32 else 8                # channels per 16-byte chunk


def _randn(shape, dtype, seed, offset=True):
    g = torch.Generator().manual_seed(seed)
    ch = torch.arange(shape[-1], dtype=torch.float32)
    t = torch.randn(*shape, generator=g) * (0.5 + (ch % 3) / 2)
    return (t + torch.sin(ch) if offset else t).to(dtype)


def _resize(dtype, c, sizes, pad=0, c0s=(0, 0, 0, 0)):
    A, L, st = O.abi()
    (hi, wi), (ho, wo) = sizes
    n = 2
    x = _randn((n, hi, wi, c), dtype, seed=hi * 100 + wo)
    y_ref = O.resize_bilinear(x, ho, wo)
    dy = (y_ref.float() + _randn((n, ho, wo, c), torch.float32, seed=hi * 100 + wo + 1, offset=False) * 0.5).to(dtype)   # <y, dy> well away from 0
    xs, ys, dys, dxs = (Slot(s, dtype, d, pad, c0) for s, d, c0 in zip(((n, hi, wi, c), (n, ho, wo, c), (n, ho, wo, c), (n, hi, wi, c)), (x, None, dy, None), c0s))
    A.check(L.srganfd_resize_bilinear(0, xs.view(A), ys.view(A), O.code(A, dtype), n, hi, wi, ho, wo, c, st), "resize fwd")
    A.check(L.srganfd_resize_bilinear(1, dys.view(A), dxs.view(A), O.code(A, dtype), n, hi, wi, ho, wo, c, st), "resize bwd")
    torch.cuda.synchronize()
    O.assert_stored(ys.val, y_ref, O.TOL_FWD, "resize y")
    O.assert_stored(dxs.val, O.resize_bilinear_backward(dy, hi, wi), O.TOL_BWD, "resize dx")
    xs.assert_untouched("x")
    dys.assert_untouched("dy")
    ys.assert_outside_untouched("y")
    dxs.assert_outside_untouched("dx")
    return x, dy, ys.val.cpu(), dxs.val.cpu()


@pytest.mark.parametrize("sizes", O.RESIZE_PAIRS, ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
@pytest.mark.parametrize("c", [8, 64])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_resize_bilinear_forward_and_backward(dtype, c, sizes):
    """identity, one source pixel, one output pixel, the extreme ratios where the backward's gather window is widest, odd ratios"""
    x, dy, y, dx = _resize(dtype, c, sizes)
    if dtype == torch.float32:                               # the two kernels are adjoint to each other: <resize(x), dy> = <x, resize_bwd(dy)>
        lhs, rhs = (y.double() * dy.double()).sum().item(), (x.double() * dx.double()).sum().item()
        print(f"adjoint identity: {lhs:.9e} vs {rhs:.9e}, rel {abs(lhs - rhs) / abs(lhs):.2e}")
        assert abs(lhs - rhs) <= 1e-5 * abs(lhs)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_resize_bilinear_on_channel_slices(dtype):
    _resize(dtype, 64, ((9, 13), (17, 33)), pad=32, c0s=(16, 8, 24, 0))


@pytest.mark.parametrize("c", [8, 64])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_add_relu_on_channel_slices(dtype, c):
    A, L, st = O.abi()
    npix = 210
    a, b = _randn((npix, c), dtype, seed=c), _randn((npix, c), dtype, seed=c + 1)
    b[:7] = -a[:7]                                           # exact cancellation: +0
    sa, sb, so = (Slot((npix, c), dtype, d, 32, c0) for d, c0 in ((a, 16), (b, 8), (None, 24)))
    A.check(L.srganfd_add_relu(sa.view(A), sb.view(A), so.view(A), O.code(A, dtype), npix, c, st), "add_relu")
    torch.cuda.synchronize()
    ref = O.add_relu(a, b)
    O.assert_stored(so.val, ref, O.TOL_FWD, "add_relu")
    assert (O.bits(so.val[:7]) == 0).all()                   # +0, not -0
    assert ((so.val.double().cpu() == 0) == (ref == 0)).all() and (ref == 0).sum() > 7 * c          # the clamp is exercised beyond the planted rows
    sa.assert_untouched("a")
    sb.assert_untouched("b")
    so.assert_outside_untouched("out")


@pytest.mark.parametrize("npix", [210, 37])
@pytest.mark.parametrize("cv", [1, 2, 16, 64])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gate_multiply_forward_and_backward(dtype, cv, npix):
    """cv 16-byte chunks per pixel = lanes of one wave whose products the backward adds by shuffles: none, one step, four steps, the whole
    wave.  210 and 37 pixels leave the last block (and, at 37 x 2, the last wave) partly filled."""
    A, L, st = O.abi()
    c = cv * _vn(dtype)
    x, dy = _randn((npix, c), dtype, seed=cv), _randn((npix, c), dtype, seed=cv + 100)
    gate = torch.rand(npix, generator=torch.Generator().manual_seed(cv + 200)) + 0.25
    gd = gate.cuda()
    sx, sy, sdy, sdx = (Slot((npix, c), dtype, d, 32, c0) for d, c0 in ((x, 16), (None, 8), (dy, 8), (None, 24)))
    dgate = torch.full((npix + 8,), SENTINEL, device="cuda")
    A.check(L.srganfd_gate_mul(0, sx.view(A), gd.data_ptr(), sy.view(A), A.NULL_VIEW, None, O.code(A, dtype), npix, c, st), "gate fwd")
    A.check(L.srganfd_gate_mul(1, sx.view(A), gd.data_ptr(), sdy.view(A), sdx.view(A), dgate.data_ptr(), O.code(A, dtype), npix, c, st), "gate bwd")
    torch.cuda.synchronize()
    dx_ref, dgate_ref = O.gate_backward(x, gate, dy)
    O.assert_stored(sy.val, O.gate(x, gate), O.TOL_FWD, "gate y")
    O.assert_stored(sdx.val, dx_ref, O.TOL_BWD, "gate dx")
    O.assert_f32(dgate[:npix], dgate_ref, O.TOL_FWD, "dgate")
    assert (dgate[npix:] == SENTINEL).all()
    sx.assert_untouched("x")
    sdy.assert_untouched("dy")
    sy.assert_outside_untouched("y")
    sdx.assert_outside_untouched("dx")


@pytest.mark.parametrize("cv", [128, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gate_multiply_refuses_what_one_wave_cannot_reduce(dtype, cv):
    A, L, st = O.abi()
    npix, c = 37, cv * _vn(dtype)
    sx, sy, sdx = (Slot((npix, c), dtype, d) for d in (_randn((npix, c), dtype, seed=1), None, None))
    gate, dgate = torch.ones(npix, device="cuda"), torch.full((npix,), SENTINEL, device="cuda")
    with pytest.raises(A.SrganfdError):
        A.check(L.srganfd_gate_mul(0, sx.view(A), gate.data_ptr(), sy.view(A), A.NULL_VIEW, None, O.code(A, dtype), npix, c, st))
    with pytest.raises(A.SrganfdError):
        A.check(L.srganfd_gate_mul(1, sx.view(A), gate.data_ptr(), sx.view(A), sdx.view(A), dgate.data_ptr(), O.code(A, dtype), npix, c, st))
    torch.cuda.synchronize()
    sy.assert_untouched("y")
    sdx.assert_untouched("dx")
    assert (dgate == SENTINEL).all()


@pytest.mark.parametrize("c", [64, 3], ids=["vector", "scalar"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_maxpool_forward(dtype, c):
    A, L, st = O.abi()
    n, h, w = 2, 6, 10
    x = _randn((n, h, w, c), dtype, seed=c)
    sx, sy = Slot((n, h, w, c), dtype, x, 32, 16), Slot((n, h // 2, w // 2, c), dtype, None, 32, 8)
    A.check(L.srganfd_resample(3, sx.view(A), sy.view(A), O.code(A, dtype), n, h, w, c, st), "maxpool2")
    torch.cuda.synchronize()
    assert torch.equal(sy.val.double().cpu(), O.maxpool2(x))              # a maximum of stored values is a stored value
    sx.assert_untouched("x")
    sy.assert_outside_untouched("y")


@pytest.mark.parametrize("c", [64, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_maxpool_backward_through_relu_ties_and_dead_windows(dtype, c):
    """ties inside a window: the first maximum in row-major order takes the gradient; a window with nothing positive gets none"""
    A, L, st = O.abi()
    n, h, w = 2, 6, 10
    g = torch.Generator().manual_seed(40 + c)
    x = torch.clamp(torch.round(torch.randn(n, h, w, c, generator=g) * 2) / 2, min=0.0)     # a ReLU output on a grid of halves: ties everywhere
    x[0, 0:2, 0:2] = 0.0                                                                     # nothing positive
    x[0, 2:4, 2:4] = 0.75                                                                    # four equal maxima
    x[1, 0, 0], x[1, 0, 1], x[1, 1, 0], x[1, 1, 1] = 0.5, 2.5, 2.5, 2.5                       # the first of three
    x[1, 4, 8], x[1, 4, 9], x[1, 5, 8], x[1, 5, 9] = 0.0, 1.0, 3.0, 3.0                       # the first of the second row
    x = x.to(dtype)
    dy = _randn((n, h // 2, w // 2, c), dtype, seed=41 + c)
    sx, sdy, sdx = Slot((n, h, w, c), dtype, x, 32, 16), Slot((n, h // 2, w // 2, c), dtype, dy, 32, 8), Slot((n, h, w, c), dtype, None, 32, 24)
    A.check(L.srganfd_maxpool2_relu_bwd(sx.view(A), sdy.view(A), sdx.view(A), O.code(A, dtype), n, h, w, c, st), "maxpool2_relu_bwd")
    torch.cuda.synchronize()
    ref = O.maxpool2_relu_backward(x, dy)
    dx = sdx.val.double().cpu()
    assert torch.equal(dx, ref)
    assert (dx[0, 0:2, 0:2] == 0).all() and torch.equal(dx[0, 2, 2], dy[0, 1, 1].double()) and (dx[0, 2, 3] == 0).all() and (dx[0, 3, 2:4] == 0).all()
    assert torch.equal(dx[1, 0, 1], dy[1, 0, 0].double()) and torch.equal(dx[1, 5, 8], dy[1, 2, 4].double()) and (dx[1, 5, 9] == 0).all()
    sx.assert_untouched("x")
    sdy.assert_untouched("dy")
    sdx.assert_outside_untouched("dx")
