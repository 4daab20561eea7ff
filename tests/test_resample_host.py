"""tests/resample_oracle.py against torch's own float64 operators, under autograd where there is a gradient (no GPU): what makes the
comparisons of tests/test_resample_gpu.py and tests/test_layout_gpu.py trustworthy.  Equality to 1e-12 where something is added or
multiplied, exact where values are only selected and copied.  (The views these entry points refuse: tests/test_host_logic.py.)"""
import pytest
import torch
import torch.nn.functional as F

from tests import resample_oracle as O

RTOL = 1e-12
NAN, INF = float("nan"), float("inf")


def _close(got, want, what):
    want = want.detach().double()
    assert got.shape == want.shape, what
    e = ((got.double() - want).abs().max() / (want.abs().max() + 1e-300)).item()
    assert e <= RTOL, f"{what}: {e:.3e}"


def _same(got, want, what):
    """exactly the same values, the sign of a zero and the place of every NaN included"""
    got, want = got.double(), want.detach().double()
    assert got.shape == want.shape, what
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan) and torch.equal(got[~nan], want[~nan]) and torch.equal(torch.signbit(got), torch.signbit(want)), what


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _shape(shape):
    return O.x2_shape(shape, torch.float32)


@pytest.mark.parametrize("shape", O.X2_SHAPES + [(1, 65536, 1, 4)], ids=O.X2_IDS + ["tall"])
def test_bilinear_x2_equals_interpolate_and_its_adjoint(shape):
    n, h, w, c = _shape(shape)
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randn(n, h, w, c, generator=g, dtype=torch.float64)
    dy = torch.randn(n, 2 * h, 2 * w, c, generator=g, dtype=torch.float64)
    act = torch.randn(n, h, w, c, generator=g, dtype=torch.float64)
    act[0, 0, 0, :2] = 0.0                                              # LeakyReLU'(0) is the slope
    xt = _nchw(x).clone().requires_grad_(True)
    yt = F.interpolate(xt, scale_factor=2, mode="bilinear", align_corners=False)
    yt.backward(_nchw(dy))
    y, dx = O.bilinear_up2(x), O.bilinear_up2_backward(dy)
    _close(_nchw(y), yt, "y")
    _close(_nchw(dx), xt.grad, "dx")
    if h <= 64:                                                         # the closed form is the matrix of tests/norm_oracle.py
        my, mx = O.resize_matrix(h, 2 * h), O.resize_matrix(w, 2 * w)
        _close(y, torch.einsum("yh,xw,nhwc->nyxc", my, mx, x), "y by the matrix")
        _close(dx, torch.einsum("yh,xw,nyxc->nhwc", my, mx, dy), "dx by the matrix")
    lhs, rhs = (y * dy).sum().item(), (x * dx).sum().item()
    assert abs(lhs - rhs) <= RTOL * (y * dy).abs().sum().item()
    # through the LeakyReLU in front of the upsampling: u = leaky_relu(z), act = u
    z = torch.where(act > 0, act, act / 0.2)
    zt = _nchw(z).clone().requires_grad_(True)
    F.interpolate(F.leaky_relu(zt, 0.2), scale_factor=2, mode="bilinear", align_corners=False).backward(_nchw(dy))
    raw, masked = O.bilinear_up2_backward(dy, act, 0.2)
    assert torch.equal(raw, dx)
    _close(_nchw(masked), zt.grad, "dx masked")
    assert torch.equal(masked[0, 0, 0, :2], 0.2 * dx[0, 0, 0, :2])


def test_the_x2_matrix_holds_the_kernels_taps():
    """.25 / .75, and at both ends the clamped tap folded into the edge pixel: weight 1"""
    m = O.resize_matrix(3, 6)
    want = torch.tensor([[1, 0, 0], [.75, .25, 0], [.25, .75, 0], [0, .75, .25], [0, .25, .75], [0, 0, 1]], dtype=torch.float64)
    assert torch.equal(m, want)
    assert torch.equal(O.resize_matrix(1, 2), torch.ones(2, 1, dtype=torch.float64))


def _closed_form_adjoint_taps(k, n):
    """csrc/resample.hip's bil_bwd_taps4: low-res k collects high-res 2k-1 .. 2k+2 with (.25, .75, .75, .25); a tap outside [0, 2n) is
    dropped, and the end that loses one to the clamp takes its inner neighbour with weight 1"""
    wt = [0.25, 0.75, 0.75, 0.25]
    if k == 0:
        wt[1] = 1.0
    if k == n - 1:
        wt[2] = 1.0
    return [(2 * k - 1 + j, wt[j]) for j in range(4) if 0 <= 2 * k - 1 + j < 2 * n]


@pytest.mark.parametrize("n", [1, 2, 3, 7])
def test_the_adjoints_weights_are_the_kernels_closed_form_tap_table(n):
    """the sizes at which a row meets both borders (1), one border in every row (2), and one border or none (3, 7)"""
    want = torch.zeros(n, 2 * n, dtype=torch.float64)
    for k in range(n):
        for d, w in _closed_form_adjoint_taps(k, n):
            want[k, d] = w
    got = O._up2_axis_adjoint(torch.eye(2 * n, dtype=torch.float64), 0)          # column d: what high-res d gives to each low-res k
    assert torch.equal(got, want)
    assert torch.equal(got, O.resize_matrix(n, 2 * n).T)
    borders = [sum(1 for k in range(n) for d, w in _closed_form_adjoint_taps(k, n) if w == 1.0 and k == e) for e in (0, n - 1)]
    assert borders == ([2, 2] if n == 1 else [1, 1])


@pytest.mark.parametrize("shape", O.X2_SHAPES, ids=O.X2_IDS)
def test_nearest_x2_backward_equals_autograd(shape):
    n, h, w, c = _shape(shape)
    g = torch.Generator().manual_seed(h * 100 + w + 7)
    x = torch.randn(n, h, w, c, generator=g, dtype=torch.float64)
    dy = torch.randn(n, 2 * h, 2 * w, c, generator=g, dtype=torch.float64)
    xt = _nchw(x).clone().requires_grad_(True)
    yt = F.interpolate(xt, scale_factor=2, mode="nearest")
    yt.backward(_nchw(dy))
    assert torch.equal(_nchw(O.nearest_up2(x)), yt.detach())
    _close(_nchw(O.nearest_up2_backward(dy)), xt.grad, "dx")


def test_relu_is_torchs_on_zeros_nans_and_infinities():
    g = torch.Generator().manual_seed(3)
    for dt in O.DTYPES + [torch.float64]:
        x = torch.randn(2, 6, 10, 8, generator=g).to(dt)
        x[0, 0, 0] = torch.tensor([-0.0, 0.0, NAN, INF, -INF, -1.0, 2.0, -NAN]).to(dt)
        _same(O.relu(x), F.relu(x), f"relu {dt}")
    r = O.relu(torch.tensor([-0.0, 0.0, NAN, -INF]))
    assert torch.signbit(r).tolist() == [True, False, False, False] and torch.isnan(r).tolist() == [False, False, True, False]   # -0 stays, NaN stays


@pytest.mark.parametrize("hw", [(6, 10), (7, 11), (2, 2), (3, 2)])
def test_maxpool_equals_max_pool2d_with_floor_on_odd_sizes(hw):
    h, w = hw
    g = torch.Generator().manual_seed(h)
    x = torch.round(torch.randn(2, h, w, 5, generator=g, dtype=torch.float64) * 2) / 2          # ties
    y = O.maxpool2(x)
    assert y.shape == (2, h // 2, w // 2, 5)
    assert torch.equal(_nchw(y), F.max_pool2d(_nchw(x), 2, 2))


def _special(dtype=torch.float64):
    """values around and at the ends of [0, 1]: exactly 0, exactly 1, -0, NaN, both infinities, one fp32 step outside either end"""
    return torch.tensor(O.SPECIAL, dtype=dtype)


def _layout_input(c, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(O.LAYOUT_N, c, O.LAYOUT_H, O.LAYOUT_W, generator=g)


@pytest.mark.parametrize("c,cpad", [(1, 4), (3, 4), (4, 4), (3, 32), (32, 32), (3, 6)])
def test_nchw_to_nhwc_is_permute_pad_and_normalize(c, cpad):
    x = _layout_input(c, c * 10 + cpad)
    y = O.nchw_to_nhwc(x, cpad)
    assert y.shape == (O.LAYOUT_N, O.LAYOUT_H, O.LAYOUT_W, cpad)
    assert torch.equal(y[..., :c], x.double().permute(0, 2, 3, 1))
    assert (y[..., c:] == 0).all() and not torch.signbit(y[..., c:]).any()
    mean, std = torch.linspace(0.4, 0.5, c), torch.linspace(0.22, 0.23, c)
    yn = O.nchw_to_nhwc(x, cpad, mean, std)
    _close(yn[..., :c], ((x.double() - mean.double().view(1, c, 1, 1)) / std.double().view(1, c, 1, 1)).permute(0, 2, 3, 1), "normalized")
    assert (yn[..., c:] == 0).all()


@pytest.mark.parametrize("clamp01", [0, 1])
def test_nhwc_to_nchw_is_permute_and_torchs_clamp(clamp01):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(O.LAYOUT_N, O.LAYOUT_H, O.LAYOUT_W, 3, generator=g, dtype=torch.float64) * 0.8 + 0.5
    sp = _special()
    x[0, 0, :len(sp), 1] = sp
    want = x.permute(0, 3, 1, 2)
    if clamp01:
        want = torch.clamp(want, 0, 1)
        assert torch.isnan(want[0, 1, 0, 3]) and torch.signbit(want[0, 1, 0, 2]) and want[0, 1, 0, 4] == 1 and want[0, 1, 0, 5] == 0
    _same(O.nhwc_to_nchw(x, clamp01), want, "nhwc_to_nchw")
    for dt in O.DTYPES:                                      # the clamp of a value of any type, as the kernel sees it
        _same(O.nhwc_to_nchw(x.to(dt), clamp01), torch.clamp(x.to(dt).float(), 0, 1).permute(0, 3, 1, 2) if clamp01 else x.to(dt).permute(0, 3, 1, 2), f"{dt}")


@pytest.mark.parametrize("c,cpad", [(1, 4), (3, 4), (4, 4), (3, 32), (3, 16)])
def test_clamp_grad_equals_the_gradient_of_clamp(c, cpad):
    g = torch.Generator().manual_seed(c + cpad)
    n, h, w = O.LAYOUT_N, O.LAYOUT_H, O.LAYOUT_W
    pre = torch.randn(n, h, w, c, generator=g, dtype=torch.float64) * 0.8 + 0.5
    sp = _special()
    pre[0, 0, :len(sp), c - 1] = sp
    dsr = torch.randn(n, c, h, w, generator=g, dtype=torch.float64)
    pt = pre.clone().requires_grad_(True)
    torch.clamp(_nchw(pt), 0, 1).backward(dsr)
    got = O.clamp_grad(dsr, pre, cpad)
    assert torch.equal(got[..., :c], pt.grad) and (got[..., c:] == 0).all()
    # the ends pass, -0 passes, NaN, the infinities and one step outside do not
    passed = (got[0, 0, :len(sp), c - 1] == dsr[0, c - 1, 0, :len(sp)]).tolist()
    assert passed == O.SPECIAL_INSIDE


def test_nhwc_to_nchw_scaled_is_a_division_per_channel():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(O.LAYOUT_N, O.LAYOUT_H, O.LAYOUT_W, 3, generator=g, dtype=torch.float64)
    div = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float64)
    _close(O.nhwc_to_nchw_scaled(x, div), x.permute(0, 3, 1, 2) / div.view(1, 3, 1, 1), "scaled")


def test_assert_bits_sees_one_bit_and_lets_any_nan_stand_for_another():
    a = torch.tensor([1.0, -0.0, NAN, 2.0])
    O.assert_bits(a.clone(), a, "same")
    O.assert_bits(torch.tensor([1.0, -0.0, -NAN, 2.0]), a, "another NaN")
    for other in (torch.tensor([1.0, 0.0, NAN, 2.0]), torch.tensor([1.0, -0.0, 3.0, 2.0]), torch.tensor([1.0, -0.0, NAN, 2.0000002])):
        with pytest.raises(AssertionError):
            O.assert_bits(other, a, "differs")
