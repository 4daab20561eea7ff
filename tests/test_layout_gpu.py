"""csrc/layout.hip's boundary conversions, every dispatch path of each entry point on its own against the definitions of
tests/resample_oracle.py: srganfd_nchw_to_nhwc (the NHWC4 packer, the vector and the scalar path, with and without the input
normalisation), srganfd_nhwc_to_nchw (with and without the clamp), srganfd_nhwc_to_nchw_scaled and srganfd_clamp_grad_to_nhwc (the
4-channel-pitch, the 32-channel and the generic kernel), and the second trip of the scalar grids' grid-stride loops.

Where values are only moved, rounded once or selected the result is bit for bit torch's; the normalisation and the division are held
to the bounds of tests/norm_oracle.py.  Outputs sit in channel slices between sentinels, with one more image behind the last one that
has to keep its sentinels too.

Which test reaches which launch:
  rgb_to_nhwc_kernel<T, CLAMP=0, WIDE=0>             test_nchw_to_nhwc_nhwc4_packer, test_nchw_to_nhwc4_second_trip_of_the_grid
  nchw_to_nhwc_kernel<T, N> (vector and N = 1)       test_nchw_to_nhwc_vector_path, test_nchw_to_nhwc_scalar_path,
                                                     test_nchw_to_nhwc_view_off_the_vector_takes_the_scalar_path (N = 1)
  nhwc_to_nchw_kernel                                test_nhwc_to_nchw_generator_output, _from_a_channel_slice, _second_trip_of_the_grid
  nhwc_to_nchw_scaled_kernel                         test_nhwc_to_nchw_scaled_from_a_channel_slice
  rgb_to_nhwc_kernel<T, CLAMP=1, WIDE=0 / 1>, clamp_grad_kernel       test_clamp_grad_three_paths_agree_with_the_definition_and_each_other,
                                                     test_clamp_grad_generic_path_in_fp32, test_clamp_grad_rgb4_second_trip_of_the_grid"""
import pytest
import torch

from tests import resample_oracle as O

pytestmark = pytest.mark.gpu

DTYPES, IDS, Slot, SENTINEL = O.DTYPES, O.IDS, O.Slot, O.SENTINEL
BITS16 = [torch.bfloat16, torch.float16]
N, H, W = O.LAYOUT_N, O.LAYOUT_H, O.LAYOUT_W
GRID = 8192 * 256                                            # threads of the largest scalar grid: one element more takes a second trip
STD = [0.229, 0.224, 0.225]
# fp32 values half way between two neighbours of either 16-bit type, where round-to-nearest-even goes down and where it goes up
TIES = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -11)]


def _out_slot(n, h, w, cpad, dtype, pad, c0):
    """an output slot with one image more than the call is told about"""
    return Slot((n + 1, h, w, cpad), dtype, None, pad, c0)


def _nchw_input(n, c, h, w, seed):
    x = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(seed))
    flat = x.view(-1)
    flat[:len(TIES)] = torch.tensor(TIES)
    flat[-len(TIES):] = torch.tensor(TIES)
    return x


def _nchw_to_nhwc(dtype, c, cpad, pad, c0, norm, n=N, h=H, w=W, seed=0):
    A, L, st = O.abi()
    x = _nchw_input(n, c, h, w, seed + c * 100 + cpad)
    xd = x.cuda()
    before = xd.clone()
    mean, std = (torch.linspace(0.4, 0.5, c), torch.linspace(0.22, 0.23, c)) if norm else (None, None)
    md, sd = (mean.cuda(), std.cuda()) if norm else (None, None)
    out = _out_slot(n, h, w, cpad, dtype, pad, c0)
    A.check(L.srganfd_nchw_to_nhwc(xd.data_ptr(), n, c, h, w, out.view(A), O.code(A, dtype), cpad, md.data_ptr() if norm else None, sd.data_ptr() if norm else None, st), "nchw_to_nhwc")
    torch.cuda.synchronize()
    assert torch.equal(xd, before)
    out.assert_outside_untouched("nchw_to_nhwc")
    assert (out.val[n] == SENTINEL).all(), "the image behind the last one was written"
    got = out.val[:n]
    assert (O.bits(got[..., c:]) == 0).all(), "padding channels are not +0"
    if norm:
        O.assert_stored(got, O.nchw_to_nhwc(x, cpad, mean, std), O.TOL_FWD, "nchw_to_nhwc normalised")
    else:
        O.assert_bits(got[..., :c], x.permute(0, 2, 3, 1).to(dtype), "nchw_to_nhwc")
        O.assert_bits(got, O.nchw_to_nhwc(x, cpad).to(dtype), "nchw_to_nhwc against the definition")
    return got


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "normalised"])
@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("dtype", BITS16, ids=IDS[1:])
def test_nchw_to_nhwc_nhwc4_packer(dtype, c, norm):
    """16-bit, at most 4 channels into a buffer of 4: one 8-byte store per pixel"""
    _nchw_to_nhwc(dtype, c, 4, 0, 0, norm)


# (c, cpad, pad, c0): 3 channels padded to 32; 32 channels at channel 8 of a 64-wide buffer; fp32 alone: 3 padded to a pitch of 4 (16-bit: the packer's)
VECTOR_CASES = [(dt, case) for dt in DTYPES for case in ((3, 32, 0, 0), (32, 32, 32, 8))] + [(torch.float32, (3, 4, 0, 0))]
VECTOR_IDS = ["%s-%dto%dat%d" % (IDS[DTYPES.index(dt)], case[0], case[1], case[3]) for dt, case in VECTOR_CASES]


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "normalised"])
@pytest.mark.parametrize("dtype,case", VECTOR_CASES, ids=VECTOR_IDS)
def test_nchw_to_nhwc_vector_path(dtype, case, norm):
    c, cpad, pad, c0 = case
    _nchw_to_nhwc(dtype, c, cpad, pad, c0, norm)


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "normalised"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_nchw_to_nhwc_scalar_path(dtype, norm):
    """fp32 padded to 6 channels (no multiple of a vector), 16-bit at a channel offset of 4"""
    if dtype == torch.float32:
        _nchw_to_nhwc(dtype, 3, 6, 2, 1, norm)
    else:
        _nchw_to_nhwc(dtype, 3, 8, 8, 4, norm)


@pytest.mark.parametrize("how", ["c0 one channel off", "cstride off the vector"])
@pytest.mark.parametrize("norm", [False, True], ids=["plain", "normalised"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_nchw_to_nhwc_view_off_the_vector_takes_the_scalar_path(dtype, norm, how):
    """cpad two whole vectors and the base pointer aligned; the view alone is off: it starts one channel into its buffer, or its buffer is
    one channel wider than a multiple of the vector (every pixel but the first is then off 16 bytes)"""
    v = O.vn(dtype)
    pad, c0 = (v, 1) if how.startswith("c0") else (v + 1, v)
    _nchw_to_nhwc(dtype, 3, 2 * v, pad, c0, norm)


# ---- NHWC -> NCHW ----
def _planted(shape, dtype, seed, scale=0.8):
    """NHWC values around [0, 1] with resample_oracle.SPECIAL in the first pixels of the first and of the last channel"""
    x = (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + 0.5).to(dtype)
    sp = torch.tensor(O.SPECIAL).to(dtype)
    x[0, 0, :len(sp), 0] = sp
    x[-1, -1, -len(sp):, -1] = sp
    return x


def _nhwc_to_nchw(dtype, c, pad, c0, clamp01, n=N, h=H, w=W):
    A, L, st = O.abi()
    x = _planted((n, h, w, c), dtype, seed=c + clamp01)
    src = Slot((n, h, w, c), dtype, x, pad, c0)
    dst = torch.full((n + 1, c, h, w), SENTINEL, device="cuda")
    A.check(L.srganfd_nhwc_to_nchw(src.view(A), O.code(A, dtype), n, c, h, w, dst.data_ptr(), clamp01, st), "nhwc_to_nchw")
    torch.cuda.synchronize()
    src.assert_untouched("nhwc_to_nchw source")
    assert (dst[n] == SENTINEL).all()
    want = x.float().permute(0, 3, 1, 2).contiguous()
    if clamp01:
        want = torch.clamp(want, 0, 1)
        assert torch.isnan(want).sum() == 2 and torch.signbit(want[0, 0, 0, 2]) and want[0, 0, 0, 2] == 0
    O.assert_bits(dst[:n], want, "nhwc_to_nchw")
    O.assert_bits(dst[:n], O.nhwc_to_nchw(x, clamp01).float(), "nhwc_to_nchw against the definition")


def test_nhwc_to_nchw_generator_output():
    """the generator's fp32 output: 3 channels at a pitch of 4, clamped (a NaN stays one, as under torch's clamp_)"""
    _nhwc_to_nchw(torch.float32, 3, 1, 0, 1)


@pytest.mark.parametrize("clamp01", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_nhwc_to_nchw_from_a_channel_slice(dtype, clamp01):
    _nhwc_to_nchw(dtype, 64, 32, 16, clamp01)


def test_nhwc_to_nchw_scaled_from_a_channel_slice():
    A, L, st = O.abi()
    c = 3
    x = torch.randn(N, H, W, c, generator=torch.Generator().manual_seed(21))
    div = torch.tensor(STD[:c])
    src = Slot((N, H, W, c), torch.float32, x, 5, 2)
    dst = torch.full((N + 1, c, H, W), SENTINEL, device="cuda")
    dd = div.cuda()
    A.check(L.srganfd_nhwc_to_nchw_scaled(src.view(A), N, c, H, W, dst.data_ptr(), dd.data_ptr(), st), "nhwc_to_nchw_scaled")
    torch.cuda.synchronize()
    src.assert_untouched("source")
    assert (dst[N] == SENTINEL).all()
    ref = O.nhwc_to_nchw_scaled(x, div)
    _, e = torch.frexp(ref.abs())
    ulp32 = torch.ldexp(torch.ones_like(ref), e - 1 - 23)                          # the spacing of fp32 at |ref|
    worst = ((dst[:N].double().cpu() - ref).abs() / ulp32).max().item()
    print(f"nhwc_to_nchw_scaled: worst error {worst:.3f} fp32 ulp")
    assert worst <= 1.0


# ---- the clamp's gradient ----
def _clamp_grad_case(n, c, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    dsr = torch.randn(n, c, h, w, generator=g) + 3.0                                # nowhere 0: a gradient that passes or not shows
    pre = torch.randn(n, h, w, 4, generator=g) * 0.8 + 0.5                          # fp32 NHWC at a pitch of 4
    sp = torch.tensor(O.SPECIAL)
    pre[0, 0, :len(sp), 0] = sp
    pre[-1, -1, -len(sp):, c - 1] = sp
    pre[..., c:] = float("nan")                                                     # channels the call does not have
    return dsr, pre


def _clamp_grad(dtype, dsr, pre, c, cpad, pad=0, c0=0):
    A, L, st = O.abi()
    n, _, h, w = dsr.shape
    dd, pd = dsr.cuda(), pre.cuda()
    d0, p0 = dd.clone(), pd.clone()
    out = _out_slot(n, h, w, cpad, dtype, pad, c0)
    A.check(L.srganfd_clamp_grad_to_nhwc(dd.data_ptr(), A.view(pd), n, c, h, w, out.view(A), O.code(A, dtype), cpad, st), "clamp_grad")
    torch.cuda.synchronize()
    assert torch.equal(dd, d0) and torch.equal(O.bits(pd), O.bits(p0))
    out.assert_outside_untouched("clamp_grad")
    assert (out.val[n] == SENTINEL).all(), "the image behind the last one was written"
    got = out.val[:n].cpu()
    O.assert_bits(got, O.clamp_grad(dsr, pre[..., :c], cpad).to(dtype), "clamp_grad against the definition")
    return got


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("dtype", BITS16, ids=IDS[1:])
def test_clamp_grad_three_paths_agree_with_the_definition_and_each_other(dtype, c):
    dsr, pre = _clamp_grad_case(N, c, H, W, seed=30 + c)
    rgb4 = _clamp_grad(dtype, dsr, pre, c, 4)
    rgb16 = _clamp_grad(dtype, dsr, pre, c, 32)
    generic = _clamp_grad(dtype, dsr, pre, c, 8, pad=8, c0=4)
    O.assert_bits(rgb16[..., :4], rgb4, "32-channel against 4-channel pitch")
    O.assert_bits(generic[..., :4], rgb4, "generic against 4-channel pitch")
    # the ends and -0 pass, a NaN, an infinity or one fp32 step outside does not
    want = dsr[0, 0, 0, :len(O.SPECIAL)].to(dtype)
    for path in (rgb4, rgb16, generic):
        passed = path[0, 0, :len(O.SPECIAL), 0]
        assert ((passed == want) == torch.tensor(O.SPECIAL_INSIDE)).all() and (passed[~torch.tensor(O.SPECIAL_INSIDE)] == 0).all()


@pytest.mark.parametrize("c", [1, 3, 4])
def test_clamp_grad_generic_path_in_fp32(c):
    dsr, pre = _clamp_grad_case(N, c, H, W, seed=40 + c)
    got = _clamp_grad(torch.float32, dsr, pre, c, 4)
    assert torch.equal(got[0, 0, :2, 0], dsr[0, 0, 0, :2])
    _clamp_grad(torch.float32, dsr, pre, c, 6, pad=3, c0=1)


# ---- past 8192 x 256 elements: the second trip of the grid-stride loop ----
def test_nhwc_to_nchw_second_trip_of_the_grid():
    """2 x 3 x 600 x 583 = 2 098 800 elements on a grid capped at 2 097 152 threads: the generator's output at full size takes three trips"""
    n, c, h, w = 2, 3, 600, 583
    assert GRID < n * c * h * w < GRID + 256 * 8
    _nhwc_to_nchw(torch.float32, c, 1, 0, 1, n=n, h=h, w=w)


def test_nchw_to_nhwc4_second_trip_of_the_grid():
    """one thread per pixel: 3601 x 583 pixels"""
    n, c, h, w = 1, 3, 3601, 583
    assert GRID < n * h * w < GRID + 256 * 16
    got = _nchw_to_nhwc(torch.float16, c, 4, 0, 0, False, n=n, h=h, w=w)
    assert got[0, -1, -1, c - 1] == torch.tensor(TIES[-1]).to(torch.float16)         # the last element, a planted tie


def test_clamp_grad_rgb4_second_trip_of_the_grid():
    n, c, h, w = 1, 3, 3601, 583
    dsr, pre = _clamp_grad_case(n, c, h, w, seed=50)
    got = _clamp_grad(torch.float16, dsr, pre, c, 4)
    assert pre[0, -1, -1, c - 1] == O.SPECIAL[-1] and got[0, -1, -1, c - 1] == dsr[0, c - 1, -1, -1].to(torch.float16)   # the last element: inside, passed
