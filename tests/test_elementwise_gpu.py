"""csrc/elementwise.hip's maps that are not fused into a conv epilogue, every launch line on its own against the float64 definitions of
tests/step_oracle.py: srganfd_lrelu_bwd (vector and scalar form, with and without skip, in place), srganfd_axpby (vector, scalar, the
flat single-channel form of the trainers), srganfd_sigmoid and srganfd_sigmoid_bwd (in place), and the second trip of their grid-stride
loops.  relu(a + b) and the gate multiply are in tests/test_attention_gate_gpu.py.

Views sit at different channel offsets of padded buffers filled with sentinels; an output buffer has one pixel more than the call is
told about.  Stored maps are held to norm_oracle.assert_stored (TOL_BWD for the backward maps, TOL_FWD for the forward ones); where a
value is only selected it is bit for bit the input.

Which test reaches which launch (SRGANFD_LAUNCH lines of csrc/elementwise.hip; N = the 16-byte vector, or 1 for the scalar form):
  lrelu_bwd_kernel<T, N>      test_lrelu_bwd_vector_form, test_lrelu_bwd_in_place, test_lrelu_bwd_forms_agree_bit_for_bit,
                              test_lrelu_bwd_one_stride_off_the_vector_takes_the_scalar_form, test_lrelu_bwd_vector_grid_second_trip
  lrelu_bwd_kernel<T, 1>      test_lrelu_bwd_scalar_form, test_lrelu_bwd_in_place, test_lrelu_bwd_forms_agree_bit_for_bit,
                              test_lrelu_bwd_one_stride_off_the_vector_takes_the_scalar_form, test_scalar_grids_second_trip
  axpby_kernel<T, N>          test_axpby_vector_form, test_axpby_forms_agree_bit_for_bit, test_axpby_one_view_off_the_vector_takes_the_scalar_form
  axpby_kernel<T, 1>          test_axpby_scalar_form, test_axpby_flat_form_of_the_trainers, test_axpby_single_element,
                              test_axpby_forms_agree_bit_for_bit, test_axpby_one_view_off_the_vector_takes_the_scalar_form,
                              test_scalar_grids_second_trip
  sigmoid_kernel              test_sigmoid_saturates_without_nan, test_scalar_grids_second_trip
  sigmoid_bwd_kernel          test_sigmoid_bwd_in_place_and_not, test_scalar_grids_second_trip
  add_relu_kernel, gate_fwd_kernel, gate_bwd_kernel             tests/test_attention_gate_gpu.py"""
import pytest
import torch

from tests import step_oracle as O

pytestmark = pytest.mark.gpu

DTYPES, IDS, Slot, SENTINEL = O.DTYPES, O.IDS, O.Slot, O.SENTINEL
GRID = 8192 * 256                                            # threads of the largest scalar grid: one element more takes a second trip
VEC_GRID = 65536 * 256                                       # 16-byte chunks of the largest vector grid
NPIX = 37 * 29                                               # a ragged pixel count, more than one block in every form


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _next_up(x):
    """the next larger value of x's own type (x > 0)"""
    it = torch.int32 if x.dtype == torch.float32 else torch.int16
    return (x.view(it) + 1).view(x.dtype)


def _tiny(dtype):
    """the smallest positive step of the type that fp32 holds as a normal number"""
    return 2.0 ** -24 if dtype == torch.float16 else 2.0 ** -126


def _lrelu_case(dtype, npix, c, with_skip, seed):
    """dy nowhere 0, so that pass or slope shows.  Planted in the first and in the last five elements: act - skip exactly 0 and -0, act
    one step of its own type above and below skip (a difference that an fp32 subtraction keeps and anything coarser loses), a NaN."""
    g = _gen(seed)
    dy = (torch.randn(npix, c, generator=g) + 3.0).to(dtype)
    act = torch.randn(npix, c, generator=g).to(dtype)
    skip = torch.randn(npix, c, generator=g).abs().add(0.5).to(dtype) if with_skip else None
    a, k = act.view(-1), (skip.view(-1) if with_skip else None)
    for i in (0, a.numel() - 5):
        if with_skip:
            k[i + 1] = 0.0
            a[i] = k[i]                                       # act - skip = +0
            a[i + 1] = -0.0                                   # -0 - 0 = -0
            a[i + 2] = _next_up(k[i + 2:i + 3])[0]            # one step above skip: positive
            a[i + 3] = k[i + 3]
            k[i + 3] = _next_up(k[i + 3:i + 4])[0]            # one step below skip: negative
        else:
            a[i:i + 4] = torch.tensor([0.0, -0.0, _tiny(dtype), -_tiny(dtype)]).to(dtype)
        a[i + 4] = float("nan")
    return dy, act, skip


def _lrelu_bwd(dtype, dy, act, skip, geo, inplace=False, slope=0.2, check=True):
    """geo: (pad, c0) of the dy, act, skip and out buffers.  Returns the output values; check=False leaves their comparison to the caller."""
    A, L, st = O.abi()
    npix, c = dy.shape
    sd = Slot((npix, c), dtype, dy, *geo[0])
    sa = Slot((npix, c), dtype, act, *geo[1])
    ss = Slot((npix, c), dtype, skip, *geo[2]) if skip is not None else None
    so = sd if inplace else Slot((npix + 1, c), dtype, None, *geo[3])
    A.check(L.srganfd_lrelu_bwd(sd.view(A), sa.view(A), ss.view(A) if ss else A.NULL_VIEW, so.view(A), O.code(A, dtype), npix, c, slope, st), "lrelu_bwd")
    torch.cuda.synchronize()
    sa.assert_untouched("act")
    if ss:
        ss.assert_untouched("skip")
    so.assert_outside_untouched("lrelu_bwd")
    if not inplace:
        sd.assert_untouched("dy")
        assert (so.val[npix] == SENTINEL).all(), "the pixel behind the last one was written"
    got = so.val[:npix]
    if check:
        O.assert_stored(got, O.lrelu_backward(dy, act, skip, O.f32(slope)), O.TOL_BWD, "lrelu_bwd")
        z = act.double() - (skip.double() if skip is not None else 0.0)
        O.assert_bits(got.cpu()[z > 0], dy[z > 0], "lrelu_bwd where the gradient passes")
    return got


# (pad, c0) of dy, act, skip, out: all at different places
def _geo(v):
    return [(2 * v, v), (v, 0), (3 * v, 2 * v), (v, v)]


@pytest.mark.parametrize("with_skip", [False, True], ids=["plain", "skip"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_lrelu_bwd_vector_form(dtype, with_skip):
    """c, every c0 and every cstride a multiple of the 16-byte vector; 3 vectors per pixel (no power of two)"""
    v = O.vn(dtype)
    dy, act, skip = _lrelu_case(dtype, NPIX, 3 * v, with_skip, seed=1)
    _lrelu_bwd(dtype, dy, act, skip, _geo(v))


@pytest.mark.parametrize("how", ["c=3", "c0 off the vector"])
@pytest.mark.parametrize("with_skip", [False, True], ids=["plain", "skip"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_lrelu_bwd_scalar_form(dtype, with_skip, how):
    v = O.vn(dtype)
    if how == "c=3":
        dy, act, skip = _lrelu_case(dtype, NPIX, 3, with_skip, seed=2)
        _lrelu_bwd(dtype, dy, act, skip, [(5, 2), (1, 0), (v - 3, 0), (2, 1)])
    else:
        dy, act, skip = _lrelu_case(dtype, NPIX, 2 * v, with_skip, seed=3)
        geo = _geo(v)
        geo[1] = (v, 1)                                       # act alone starts one channel off: every buffer's stride stays a multiple of the vector
        _lrelu_bwd(dtype, dy, act, skip, geo)


@pytest.mark.parametrize("form", ["vector", "scalar"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_lrelu_bwd_in_place(dtype, form):
    """out is dy, as the generator's backward calls it"""
    v = O.vn(dtype)
    c = 2 * v if form == "vector" else 3
    dy, act, skip = _lrelu_case(dtype, NPIX, c, True, seed=4)
    _lrelu_bwd(dtype, dy, act, skip, _geo(v) if form == "vector" else [(5, 2), (1, 0), (3, 1), None], inplace=True)
    _lrelu_bwd(dtype, dy, act, None, _geo(v) if form == "vector" else [(5, 2), (1, 0), None, None], inplace=True)


@pytest.mark.parametrize("with_skip", [False, True], ids=["plain", "skip"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_lrelu_bwd_forms_agree_bit_for_bit(dtype, with_skip):
    """the same data through the vector kernel and (one view a channel off) through the scalar kernel"""
    v = O.vn(dtype)
    dy, act, skip = _lrelu_case(dtype, NPIX, 2 * v, with_skip, seed=5)
    vec = _lrelu_bwd(dtype, dy, act, skip, _geo(v))
    geo = _geo(v)
    geo[3] = (v, 3)
    sca = _lrelu_bwd(dtype, dy, act, skip, geo)
    O.assert_bits(vec, sca, "lrelu_bwd: vector against scalar form")


@pytest.mark.parametrize("which", range(4), ids=["dy", "act", "skip", "out"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_lrelu_bwd_one_stride_off_the_vector_takes_the_scalar_form(dtype, which):
    """c and every c0 a multiple of the vector, every base pointer aligned, and exactly one buffer one channel wider than a multiple of the
    vector: its second pixel is no longer aligned, so the whole call has to take the scalar form.  Same bits as the vector form."""
    v = O.vn(dtype)
    dy, act, skip = _lrelu_case(dtype, NPIX, 2 * v, True, seed=15)
    vec = _lrelu_bwd(dtype, dy, act, skip, _geo(v))
    geo = _geo(v)
    geo[which] = (geo[which][0] + 1, geo[which][1])
    sca = _lrelu_bwd(dtype, dy, act, skip, geo)
    O.assert_bits(vec, sca, "lrelu_bwd: vector form against the scalar form a stride forces")


# ---- axpby ----
def _axpby(dtype, x, y, geo, alpha, beta, flat=False):
    A, L, st = O.abi()
    npix, c = x.shape
    sx = Slot((npix, c), dtype, x, *geo[0])
    sy = Slot((npix + 1, c), dtype, None, *geo[1])
    sy.val[:npix].copy_(y)
    sy.before = sy.buf.clone()
    A.check(L.srganfd_axpby(sx.view(A), sy.view(A), O.code(A, dtype), npix, c, alpha, beta, st), "axpby")
    torch.cuda.synchronize()
    sx.assert_untouched("x")
    sy.assert_outside_untouched("axpby")
    assert (sy.val[npix] == SENTINEL).all(), "the pixel behind the last one was written"
    got = sy.val[:npix]
    O.assert_stored(got, O.axpby(x, y, O.f32(alpha), O.f32(beta)), O.TOL_FWD, f"axpby alpha {alpha} beta {beta}")
    return got


def _axpby_case(dtype, npix, c, seed, nan_in_y=False):
    g = _gen(seed)
    x, y = torch.randn(npix, c, generator=g).to(dtype), torch.randn(npix, c, generator=g).to(dtype)
    if nan_in_y:
        y[0, 0] = y[-1, -1] = y[npix // 2, c // 2] = float("nan")
    return x, y


AB = [(0.75, -1.5), (1.0, 1.0), (2.0, 0.0)]
AB_IDS = ["general", "accumulate", "beta0-over-nan"]


@pytest.mark.parametrize("ab", AB, ids=AB_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_axpby_vector_form(dtype, ab):
    v = O.vn(dtype)
    x, y = _axpby_case(dtype, NPIX, 3 * v, seed=6, nan_in_y=ab[1] == 0.0)
    _axpby(dtype, x, y, [(2 * v, v), (v, 0)], *ab)


@pytest.mark.parametrize("ab", AB, ids=AB_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_axpby_scalar_form(dtype, ab):
    x, y = _axpby_case(dtype, NPIX, 3, seed=7, nan_in_y=ab[1] == 0.0)
    _axpby(dtype, x, y, [(5, 2), (2, 1)], *ab)


@pytest.mark.parametrize("ab", AB[:2], ids=AB_IDS[:2])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_axpby_forms_agree_bit_for_bit(dtype, ab):
    v = O.vn(dtype)
    x, y = _axpby_case(dtype, NPIX, 2 * v, seed=8)
    vec = _axpby(dtype, x, y, [(2 * v, v), (v, 0)], *ab)
    sca = _axpby(dtype, x, y, [(2 * v, v), (v, 1)], *ab)
    O.assert_bits(vec, sca, "axpby: vector against scalar form")


@pytest.mark.parametrize("how", ["c0 one channel off", "cstride off the vector"])
@pytest.mark.parametrize("which", [0, 1], ids=["x", "y"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_axpby_one_view_off_the_vector_takes_the_scalar_form(dtype, which, how):
    """c a multiple of the vector and the base pointers aligned; exactly one term of the eligibility test fails, for exactly one view"""
    v = O.vn(dtype)
    x, y = _axpby_case(dtype, NPIX, 2 * v, seed=16)
    geo = [(2 * v, v), (v, 0)]                                 # (pad, c0) of x and y: the vector form's
    vec = _axpby(dtype, x, y, geo, *AB[0])
    pad, c0 = geo[which]
    geo[which] = (pad, c0 + 1) if how.startswith("c0") else (pad + 1, c0)
    sca = _axpby(dtype, x, y, geo, *AB[0])
    O.assert_bits(vec, sca, "axpby: vector form against the scalar form one view forces")


def _axpby_flat(x, y, alpha, beta):
    """cstride = 1, c = 1 over fp32 arrays: how the trainers add one gradient to another"""
    A, L, st = O.abi()
    fx, fy = O.Fenced(x), O.Fenced(y)
    A.check(L.srganfd_axpby(A.View(fx.ptr(), 1, 0), A.View(fy.ptr(), 1, 0), A.F32, x.numel(), 1, alpha, beta, st), "axpby")
    torch.cuda.synchronize()
    fx.assert_untouched("x")
    fy.assert_fences("axpby")
    O.assert_f32(fy.val, O.axpby(x, y, O.f32(alpha), O.f32(beta)), O.TOL_FWD, "flat axpby")
    return fy.val


@pytest.mark.parametrize("ab", AB, ids=AB_IDS)
def test_axpby_flat_form_of_the_trainers(ab):
    x, y = _axpby_case(torch.float32, 1001, 1, seed=9, nan_in_y=ab[1] == 0.0)
    _axpby_flat(x.view(-1), y.view(-1), *ab)


def test_axpby_single_element():
    """the content loss weighted into its slot: one element, beta = 0 over whatever the slot held"""
    got = _axpby_flat(torch.tensor([0.37]), torch.tensor([float("nan")]), 0.006, 0.0)
    assert got.item() == (torch.tensor(0.37) * torch.tensor(0.006)).item()


# ---- sigmoid ----
SIG_POINTS = [0.0, -0.0, 1e-3, -1e-3, 20.0, -20.0, 90.0, -90.0, 104.0, -104.0]


def test_sigmoid_saturates_without_nan():
    A, L, st = O.abi()
    x = torch.cat([torch.tensor(SIG_POINTS), torch.randn(1001 - len(SIG_POINTS), generator=_gen(10)) * 6])
    f = O.Fenced(x)
    A.check(L.srganfd_sigmoid(f.ptr(), x.numel(), st), "sigmoid")
    torch.cuda.synchronize()
    f.assert_fences("sigmoid")
    got = f.val.cpu()
    O.assert_f32(f.val, O.sigmoid(x), O.TOL_FWD, "sigmoid")
    k = len(SIG_POINTS)
    assert got[0] == 0.5 and got[1] == 0.5 and got[2] > 0.5 > got[3]
    assert (got[[4, 6, 8]] == 1.0).all(), "the positive side saturates at 1"
    assert (got[[5, 7, 9]] >= 0).all() and got[5] > 1e-9 and (got[[7, 9]] <= 2.0 ** -126).all(), "the negative side goes to 0"
    assert ((got[:k] >= 0) & (got[:k] <= 1)).all()


@pytest.mark.parametrize("inplace", [False, True], ids=["out", "in-place"])
def test_sigmoid_bwd_in_place_and_not(inplace):
    """out is ds, as the attention discriminator's backward calls it"""
    A, L, st = O.abi()
    x = torch.cat([torch.tensor(SIG_POINTS), torch.randn(1001 - len(SIG_POINTS), generator=_gen(11)) * 6])
    s = O.sigmoid(x).float()
    assert s[6] == 1.0 and s[9] == 0.0
    ds = torch.randn(1001, generator=_gen(12)) + 3.0
    fd, fs = O.Fenced(ds), O.Fenced(s)
    fo = fd if inplace else O.Fenced(n=1001)
    A.check(L.srganfd_sigmoid_bwd(fd.ptr(), fs.ptr(), fo.ptr(), 1001, st), "sigmoid_bwd")
    torch.cuda.synchronize()
    fs.assert_untouched("s")
    fo.assert_fences("sigmoid_bwd")
    if not inplace:
        fd.assert_untouched("ds")
    O.assert_f32(fo.val, O.sigmoid_backward(ds, s), O.TOL_BWD, "sigmoid_bwd")
    assert fo.val[6] == 0 and fo.val[9] == 0 and fo.val[0] == ds[0] * 0.25


# ---- past the largest grid: the second trip of the grid-stride loops, the telling values in the last elements ----
def test_scalar_grids_second_trip():
    """2 097 152 + 37 elements on grids capped at 8192 blocks of 256: lrelu_bwd and axpby with c = 1, sigmoid, sigmoid_bwd"""
    A, L, st = O.abi()
    n = GRID + 37
    g = torch.Generator(device="cuda").manual_seed(13)
    tail = torch.tensor([0.0, -0.0, 1e-3, -1e-3, 20.0, -20.0, 90.0, -90.0], device="cuda")
    x = torch.randn(n, device="cuda", generator=g)
    x[-len(tail):] = tail
    dy = torch.randn(n, device="cuda", generator=g) + 3.0
    # lrelu_bwd, in place, one channel
    got = _lrelu_bwd(torch.float32, dy.view(n, 1), x.view(n, 1), None, [(0, 0), (0, 0), None, None], inplace=True, check=False)
    ref = O.lrelu_backward(dy.view(n, 1), x.view(n, 1), None, O.f32(0.2))
    O.assert_f32(got, ref, O.TOL_BWD, "lrelu_bwd, second trip")
    assert torch.equal(got[-8:, 0].cpu(), (dy[-8:] * torch.tensor([0.2, 0.2, 1, 0.2, 1, 0.2, 1, 0.2], device="cuda")).cpu())
    # axpby, flat
    fx, fy = O.Fenced(x), O.Fenced(dy)
    A.check(L.srganfd_axpby(A.View(fx.ptr(), 1, 0), A.View(fy.ptr(), 1, 0), A.F32, n, 1, 0.75, -1.5, st), "axpby")
    torch.cuda.synchronize()
    fy.assert_fences("axpby")
    O.assert_f32(fy.val, O.axpby(x, dy, 0.75, -1.5), O.TOL_FWD, "axpby, second trip")
    # sigmoid and its backward
    f = O.Fenced(x)
    A.check(L.srganfd_sigmoid(f.ptr(), n, st), "sigmoid")
    torch.cuda.synchronize()
    f.assert_fences("sigmoid")
    O.assert_f32(f.val, O.sigmoid(x), O.TOL_FWD, "sigmoid, second trip")
    assert f.val[-8] == 0.5 and f.val[-2] == 1.0 and f.val[-1] <= 2.0 ** -126 and torch.isfinite(f.val[-8:]).all()
    s = f.val.clone()
    fd = O.Fenced(dy)
    A.check(L.srganfd_sigmoid_bwd(fd.ptr(), f.ptr(), fd.ptr(), n, st), "sigmoid_bwd")
    torch.cuda.synchronize()
    fd.assert_fences("sigmoid_bwd")
    f.assert_fences("sigmoid_bwd s")
    assert torch.equal(f.val, s)
    O.assert_f32(fd.val, O.sigmoid_backward(dy, s), O.TOL_BWD, "sigmoid_bwd, second trip")
    assert fd.val[-8] == dy[-8] * 0.25 and fd.val[-2] == 0


def test_lrelu_bwd_vector_grid_second_trip():
    """f16, 8 channels, in place: 16 777 216 + 5 pixels of one 16-byte chunk each on a grid capped at 65 536 blocks; the last 5 pixels are
    the second trip's, and hold the planted values.  The reference is computed on the device in chunks."""
    A, L, st = O.abi()
    npix, c, dt = VEC_GRID + 5, 8, torch.float16
    g = torch.Generator(device="cuda").manual_seed(14)
    dy = torch.empty(npix + 1, c, dtype=dt, device="cuda")
    act = torch.empty(npix, c, dtype=dt, device="cuda")
    step = 1 << 21
    for lo in range(0, npix, step):
        hi = min(lo + step, npix)
        dy[lo:hi] = (torch.randn(hi - lo, c, device="cuda", generator=g) + 3.0).to(dt)
        act[lo:hi] = torch.randn(hi - lo, c, device="cuda", generator=g).to(dt)
    dy[npix] = SENTINEL
    act[-5:, :4] = torch.tensor([0.0, -0.0, 2.0 ** -24, -(2.0 ** -24)], dtype=dt, device="cuda")
    act[-5:, 4] = float("nan")
    dy0, act0 = dy.clone(), act.clone()
    v = A.view(dy)
    A.check(L.srganfd_lrelu_bwd(v, A.view(act), A.NULL_VIEW, v, A.F16, npix, c, 0.2, st), "lrelu_bwd")
    torch.cuda.synchronize()
    assert torch.equal(O.bits(act), O.bits(act0)) and (dy[npix] == SENTINEL).all()
    worst = -1.0
    for lo in range(0, npix, step):
        hi = min(lo + step, npix)
        ref = O.lrelu_backward(dy0[lo:hi], act0[lo:hi], None, O.f32(0.2))
        got = dy[lo:hi].double()
        assert torch.isfinite(got).all()
        # assert_stored's bound with max|ref| taken per chunk (smaller than the whole tensor's: no looser)
        excess = ((got - ref).abs() - O.ulp(ref, dt) - O.TOL_BWD * ref.abs().max()).max().item()
        worst = max(worst, excess)
        passed = act0[lo:hi].double() > 0
        assert torch.equal(O.bits(dy[lo:hi])[passed], O.bits(dy0[lo:hi])[passed])
    print(f"lrelu_bwd, vector grid's second trip: max excess over one f16 ulp + {O.TOL_BWD:.0e} max|ref|: {worst:.2e}")
    assert worst <= 0.0
    want = dy0[npix - 5:npix].double()
    mask = torch.tensor([0.2, 0.2, 1.0, 0.2, 0.2], device="cuda", dtype=torch.float64)
    tail = dy[npix - 5:npix].double()
    assert ((tail[:, :5] - want[:, :5] * mask).abs() <= O.ulp(want[:, :5] * mask, dt)).all() and torch.equal(tail[:, 2], want[:, 2])
