"""csrc/resample.hip's x2 kernels, each form of each op on its own against the float64 definitions of tests/resample_oracle.py:
srganfd_resample's ops 0-4 (adjoint of nearest x2, bilinear x2 and its adjoint, 2x2 max-pool, the ReLU copy) in the row-grid, the
generic vector and the scalar forms, and srganfd_resample_bwd_lrelu with its non-temporal twin.  Every dtype, channel-slice views with
sentinels around them, the shapes of resample_oracle.X2_SHAPES.

Bounds as in tests/test_norm_gpu.py: fp32 within 1e-5 (forward) / 1e-4 (adjoints) of float64 relative to max|ref|, a stored 16-bit
result within one ulp of its type on top of that (the x2 weights are exact in fp32 and at most 16 terms are added); max-pool and the
ReLU copy bit for bit.

Which launch of srganfd_resample and srganfd_resample_bwd_lrelu a test reaches is part of the test: every call below names the kernel
label it expects (VECTOR, SCALAR, GENERIC, ROWS_BWD_NT), and the helpers hold ops.resample_describe to it at the very arguments they
then launch with.  tests/test_resample_dispatch_host.py holds the set of labels and the thresholds between them."""
import pytest
import torch

from tests import resample_oracle as O

pytestmark = pytest.mark.gpu

DTYPES, IDS, Slot = O.DTYPES, O.IDS, O.Slot
NAN = float("nan")
OPS = {0: "nearest_bwd", 1: "bilinear_fwd", 2: "bilinear_bwd", 3: "maxpool", 4: "relu"}
TALL = 65536                                                 # more rows than a grid's y extent: the bilinear ops leave the row-grid kernels
# the labels of csrc/resample.hip's dispatch table, per op: what 16-byte views reach, what other views reach, and what the two
# bilinear ops fall back to on vectors where the row grid does not fit
VECTOR = {0: "resample_kernel<op0,vec>", 1: "bilinear_up2_rows_kernel", 2: "bilinear_up2_bwd_rows_kernel", 3: "resample_kernel<op3,vec>",
          4: "resample_kernel<op4,vec>"}
SCALAR = {op: f"resample_kernel<op{op},scalar>" for op in range(5)}
GENERIC = {1: "resample_kernel<op1,vec>", 2: "resample_kernel<op2,vec>"}
ROWS_BWD_NT = "bilinear_up2_bwd_rows_kernel<NT>"
LABELS = sorted(set(VECTOR.values()) | set(SCALAR.values()) | set(GENERIC.values()) | {ROWS_BWD_NT})


def _assert_reaches(kernel, dtype, n, h, w, c, a, b, op=None, **fused):
    """the call about to be made launches the instantiation `kernel` for `dtype`"""
    from sr_gan_fd_amd import ops
    A = O.abi()[0]
    got = ops.resample_describe(O.code(A, dtype), n, h, w, c, a, b, op, **fused)
    assert got == f"{kernel}/{IDS[DTYPES.index(dtype)]}", got


def _randn(shape, dtype, seed, offset=True):
    g = torch.Generator().manual_seed(seed)
    ch = torch.arange(shape[-1], dtype=torch.float32)
    t = torch.randn(*shape, generator=g) * (0.5 + (ch % 3) / 2)
    return (t + torch.sin(ch) if offset else t).to(dtype)


def _shapes(op, n, h, w, c):
    """(input, output) shapes of an op at (h, w): the low-resolution side for ops 0-2, the input for ops 3-4"""
    hi, lo = (n, 2 * h, 2 * w, c), (n, h, w, c)
    return {0: (hi, lo), 1: (lo, hi), 2: (hi, lo), 3: (lo, (n, h // 2, w // 2, c)), 4: (lo, lo)}[op]


REF = {0: O.nearest_up2_backward, 1: O.bilinear_up2, 2: O.bilinear_up2_backward, 3: O.maxpool2, 4: O.relu}
TOL = {0: O.TOL_BWD, 1: O.TOL_FWD, 2: O.TOL_BWD}


def _resample(reaches, op, dtype, x, out_shape, pad=32, c0s=(16, 8), h=None, w=None):
    """one srganfd_resample call through two slots, which must reach the kernel `reaches`; returns the output slot after the fences are checked"""
    A, L, st = O.abi()
    n, c = x.shape[0], x.shape[-1]
    sx, sy = Slot(x.shape, dtype, x, pad, c0s[0]), Slot(out_shape, dtype, None, pad, c0s[1])
    _assert_reaches(reaches, dtype, n, h, w, c, sx.view(A), sy.view(A), op)
    A.check(L.srganfd_resample(op, sx.view(A), sy.view(A), O.code(A, dtype), n, h, w, c, st), OPS[op])
    torch.cuda.synchronize()
    sx.assert_untouched(OPS[op] + " input")
    sy.assert_outside_untouched(OPS[op] + " output")
    return sy


def _check(op, dtype, x, got, what):
    ref = REF[op](x)
    assert tuple(got.shape) == tuple(ref.shape)
    if op in TOL:
        O.assert_stored(got, ref, TOL[op], what)
    else:
        O.assert_bits(got, ref.to(dtype), what)              # a stored value selected: exact


def _input(op, dtype, n, h, w, c, seed=0):
    return _randn(_shapes(op, n, h, w, c)[0], dtype, seed=seed + 1000 * op + h * 100 + w)


# ---- the vector forms: op 0 generic, ops 1 and 2 on the row grid ----
@pytest.mark.parametrize("shape", O.X2_SHAPES, ids=O.X2_IDS)
@pytest.mark.parametrize("op", [0, 1, 2], ids=[OPS[o] for o in (0, 1, 2)])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_x2_ops_on_channel_slices(dtype, op, shape):
    n, h, w, c = O.x2_shape(shape, dtype)
    x = _input(op, dtype, n, h, w, c)
    sy = _resample(VECTOR[op], op, dtype, x, _shapes(op, n, h, w, c)[1], h=h, w=w)
    _check(op, dtype, x, sy.val, f"{OPS[op]} {shape}")


@pytest.mark.parametrize("shape", O.X2_SHAPES, ids=O.X2_IDS)
def test_x2_ops_are_adjoint_to_their_forward_passes_in_fp32(shape):
    """<up2(x), dy> = <x, up2_bwd(dy)> for the bilinear pair of kernels, and for op 0 against repeat_interleave; dy = up2(x) + noise keeps
    the inner product well away from 0"""
    dtype = torch.float32
    n, h, w, c = O.x2_shape(shape, dtype)
    x = _randn((n, h, w, c), dtype, seed=h * 100 + w)
    noise = _randn((n, 2 * h, 2 * w, c), dtype, seed=h * 100 + w + 1, offset=False) * 0.5
    y = _resample(VECTOR[1], 1, dtype, x, (n, 2 * h, 2 * w, c), h=h, w=w).val.cpu()
    for op, fwd in ((2, y), (0, O.nearest_up2(x).float())):
        dy = (fwd + noise).to(dtype)
        dx = _resample(VECTOR[op], op, dtype, dy, (n, h, w, c), h=h, w=w).val.cpu()
        lhs, rhs = (fwd.double() * dy.double()).sum().item(), (x.double() * dx.double()).sum().item()
        print(f"{OPS[op]} adjoint identity: {lhs:.9e} vs {rhs:.9e}, rel {abs(lhs - rhs) / abs(lhs):.2e}")
        assert abs(lhs - rhs) <= 1e-5 * abs(lhs)


# ---- srganfd_resample_bwd_lrelu on the row grid ----
def _bwd_lrelu(reaches, dtype, dy, act, n, h, w, c, raw=True, slope=0.2, pad=32, c0s=(16, 8, 24, 0)):
    A, L, st = O.abi()
    lo = (n, h, w, c)
    sdy, sact, smask = Slot(dy.shape, dtype, dy, pad, c0s[0]), Slot(lo, dtype, act, pad, c0s[1]), Slot(lo, dtype, None, pad, c0s[2])
    sraw = Slot(lo, dtype, None, pad, c0s[3]) if raw else None
    _assert_reaches(reaches, dtype, n, h, w, c, sdy.view(A), sraw.view(A) if raw else A.NULL_VIEW, act=sact.view(A), b2=smask.view(A))
    A.check(L.srganfd_resample_bwd_lrelu(sdy.view(A), sraw.view(A) if raw else A.NULL_VIEW, sact.view(A), smask.view(A), O.code(A, dtype), n, h, w, c, slope, st), "bwd_lrelu")
    torch.cuda.synchronize()
    sdy.assert_untouched("dy")
    sact.assert_untouched("act")
    smask.assert_outside_untouched("dx_masked")
    if raw:
        sraw.assert_outside_untouched("dx_raw")
    return (sraw.val if raw else None), smask.val


def _act(dtype, n, h, w, c, seed):
    act = _randn((n, h, w, c), dtype, seed=seed, offset=False)
    act[:, 0, 0, :2] = 0.0                                   # exact zeros count as the negative side ...
    act[-1, -1, -1, -1] = -0.0                               # ... and so does -0
    return act


@pytest.mark.parametrize("shape", O.X2_SHAPES, ids=O.X2_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_resample_bwd_lrelu_three_ways(dtype, shape):
    n, h, w, c = O.x2_shape(shape, dtype)
    dy, act = _input(2, dtype, n, h, w, c), _act(dtype, n, h, w, c, seed=h * 10 + w)
    raw, masked = _bwd_lrelu(VECTOR[2], dtype, dy, act, n, h, w, c)
    _, only = _bwd_lrelu(VECTOR[2], dtype, dy, act, n, h, w, c, raw=False)
    ref_raw, ref_masked = O.bilinear_up2_backward(dy, act, 0.2)
    O.assert_stored(raw, ref_raw, O.TOL_BWD, f"dx_raw {shape}")
    O.assert_stored(masked, ref_masked, O.TOL_BWD, f"dx_masked {shape}")
    assert (ref_masked[:, 0, 0, :2] == 0.2 * ref_raw[:, 0, 0, :2]).all() and (ref_raw[:, 0, 0, :2] != 0).all()        # the planted zeros take the slope
    O.assert_bits(only, masked, "dx_masked without dx_raw")
    O.assert_bits(raw, _resample(VECTOR[2], 2, dtype, dy, (n, h, w, c), h=h, w=w).val, "dx_raw against op 2")


# ---- the scalar forms ----
SCALAR_SHAPE = (2, 5, 13)                                    # odd both ways: op 3 drops a row and a column


@pytest.mark.parametrize("op", list(OPS), ids=list(OPS.values()))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_scalar_forms_at_three_channels(dtype, op):
    n, h, w = SCALAR_SHAPE
    x = _input(op, dtype, n, h, w, 3)
    sy = _resample(SCALAR[op], op, dtype, x, _shapes(op, n, h, w, 3)[1], h=h, w=w)
    _check(op, dtype, x, sy.val, f"scalar {OPS[op]}")


@pytest.mark.parametrize("op", list(OPS), ids=list(OPS.values()))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_scalar_forms_take_the_views_the_vector_forms_cannot(dtype, op):
    """64 channels at a channel offset that is no multiple of a 16-byte vector (16-bit: 4, fp32: 2): the scalar forms, within the same
    bounds -- and bit for bit what the vector forms give: each op is one body at two widths (for op 2 the vector form here is the
    row-grid kernel, which keeps the generic body's products and order).  Op 1 is left out: its scalar form keeps its own nested
    expression, wy0 (wx0 a + wx1 b) + wy1 (wx0 c + wx1 d), because the A-ESRGAN attention gates' one-channel fp32 maps reach it
    (engine_a.py; the launches are in tests/golden/launch_trace.json.gz) and the vector forms' fmaf chain would move their last bit."""
    n, h, w = SCALAR_SHAPE
    c, off = 64, (2 if dtype == torch.float32 else 4)
    assert off % O.vn(dtype) != 0 and (c + 32) % O.vn(dtype) == 0
    x = _input(op, dtype, n, h, w, c)
    out_shape = _shapes(op, n, h, w, c)[1]
    scalar = _resample(SCALAR[op], op, dtype, x, out_shape, c0s=(off, off), h=h, w=w).val
    _check(op, dtype, x, scalar, f"scalar {OPS[op]} at channel {off}")
    vector = _resample(VECTOR[op], op, dtype, x, out_shape, h=h, w=w).val
    _check(op, dtype, x, vector, f"vector {OPS[op]}")
    if op != 1:
        O.assert_bits(scalar, vector, f"{OPS[op]}: scalar against vector")


# ---- the generic vector forms of ops 1 and 2: more rows than the row grid takes ----
@pytest.fixture(scope="module")
def tall():
    """per dtype: inputs and float64 references of the 65536 x 1 image, made once"""
    cache = {}

    def get(dtype):
        if dtype not in cache:
            c = O.vn(dtype)
            x, dy = _randn((1, TALL, 1, c), dtype, seed=1), _randn((1, 2 * TALL, 2, c), dtype, seed=2)
            act = _act(dtype, 1, TALL, 1, c, seed=3)
            cache[dtype] = dict(c=c, x=x, dy=dy, act=act, y=O.bilinear_up2(x), dx=O.bilinear_up2_backward(dy, act, 0.2))
        return cache[dtype]
    return get


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_generic_vector_bilinear_forward_on_a_tall_image(dtype, tall):
    t = tall(dtype)
    c, x, half = t["c"], t["x"], TALL // 2
    y = _resample(GENERIC[1], 1, dtype, x, (1, 2 * TALL, 2, c), h=TALL, w=1).val
    O.assert_stored(y, t["y"], O.TOL_FWD, "generic bilinear_fwd")
    # the row-grid form on the two halves: bit-identical on every output row that does not read across the seam
    top = _resample(VECTOR[1], 1, dtype, x[:, :half], (1, TALL, 2, c), h=half, w=1).val
    bottom = _resample(VECTOR[1], 1, dtype, x[:, half:], (1, TALL, 2, c), h=half, w=1).val
    O.assert_bits(y[:, :TALL - 1], top[:, :TALL - 1], "generic against row grid, upper half")
    O.assert_bits(y[:, TALL + 1:], bottom[:, 1:], "generic against row grid, lower half")
    assert not torch.equal(y[:, TALL - 1], top[:, TALL - 1]) and not torch.equal(y[:, TALL], bottom[:, 0])       # the seam rows do differ: the halves were run apart


@pytest.mark.parametrize("fused", [False, True], ids=["resample", "bwd_lrelu"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_generic_vector_bilinear_backward_on_a_tall_image(dtype, fused, tall):
    t = tall(dtype)
    c, dy, act, half = t["c"], t["dy"], t["act"], TALL // 2

    def run(dyp, actp, h):
        reaches = GENERIC[2] if h == TALL else VECTOR[2]
        if fused:
            return _bwd_lrelu(reaches, dtype, dyp, actp, 1, h, 1, c)
        return _resample(reaches, 2, dtype, dyp, (1, h, 1, c), h=h, w=1).val, None

    raw, masked = run(dy, act, TALL)
    O.assert_stored(raw, t["dx"][0], O.TOL_BWD, "generic bilinear_bwd")
    if fused:
        O.assert_stored(masked, t["dx"][1], O.TOL_BWD, "generic bilinear_bwd masked")
    top, bottom = run(dy[:, :TALL], act[:, :half], half), run(dy[:, TALL:], act[:, half:], half)
    for k, name in ((0, "raw"), (1, "masked")):
        if k == 0 or fused:
            full = (raw, masked)[k]
            O.assert_bits(full[:, :half - 1], top[k][:, :half - 1], f"generic against row grid, upper half, {name}")
            O.assert_bits(full[:, half + 1:], bottom[k][:, 1:], f"generic against row grid, lower half, {name}")
            assert not torch.equal(full[:, half - 1], top[k][:, half - 1]) and not torch.equal(full[:, half], bottom[k][:, 0])


# ---- max-pool on odd sizes, the ReLU copy ----
@pytest.mark.parametrize("c", [64, 3], ids=["vector", "scalar"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_maxpool_floors_odd_sizes(dtype, c):
    n, h, w = 2, 7, 11
    x = _input(3, dtype, n, h, w, c)
    sy = _resample((VECTOR if c == 64 else SCALAR)[3], 3, dtype, x, (n, 3, 5, c), h=h, w=w)
    O.assert_bits(sy.val, O.maxpool2(x).to(dtype), "maxpool 7x11")
    O.assert_bits(sy.val, x[:, :6, :10].reshape(n, 3, 2, 5, 2, c).amax(dim=(2, 4)), "maxpool 7x11 without the last row and column")


def _relu_input(dtype, c):
    x = _input(4, dtype, 2, 6, 10, c)
    x[0, 0, 0, :3] = torch.tensor([-0.0, NAN, 0.0]).to(dtype)
    x[1, 5, 9, -3:] = torch.tensor([NAN, -0.0, float("-inf")]).to(dtype)
    return x


@pytest.mark.parametrize("c", [64, 3], ids=["vector", "scalar"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_relu_copy_is_torchs_relu_with_minus_zero_and_nan(dtype, c):
    """what tests/test_resample_host.py shows torch's relu to give: a NaN stays a NaN, -0 stays -0"""
    x = _relu_input(dtype, c)
    want = torch.relu(x)
    assert torch.isnan(want[0, 0, 0, 1]) and torch.signbit(want[0, 0, 0, 0]) and want[1, 5, 9, -1] == 0
    O.assert_bits(want, O.relu(x).to(dtype), "definition")
    sy = _resample((VECTOR if c == 64 else SCALAR)[4], 4, dtype, x, x.shape, h=6, w=10)
    O.assert_bits(sy.val, want, "relu copy")


@pytest.mark.parametrize("slot", ["whole_buffer", "channel_slice"])
@pytest.mark.parametrize("c", [64, 3], ids=["vector", "scalar"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_relu_copy_in_place(dtype, c, slot):
    """the content loss's call: a and b the same view (of the whole buffer there)"""
    A, L, st = O.abi()
    x = _relu_input(dtype, c)
    s = Slot(x.shape, dtype, x) if slot == "whole_buffer" else Slot(x.shape, dtype, x, 32, 16)
    _assert_reaches((VECTOR if c == 64 else SCALAR)[4], dtype, 2, 6, 10, c, s.view(A), s.view(A), 4)
    A.check(L.srganfd_resample(4, s.view(A), s.view(A), O.code(A, dtype), 2, 6, 10, c, st), "relu in place")
    torch.cuda.synchronize()
    O.assert_bits(s.val, torch.relu(x), "relu in place")
    s.assert_outside_untouched("relu in place")


# ---- the non-temporal twin of srganfd_resample_bwd_lrelu ----
def test_resample_bwd_lrelu_nontemporal_twin_is_bitwise_the_plain_kernel():
    """Results of 192 MiB or more leave through non-temporal stores (the full-size discriminator's case): the whole batch in one call
    gives the bits of two half batches, each below the threshold."""
    A, L, st = O.abi()
    torch.manual_seed(6)
    dtype, n, h, c = torch.float16, 6, 512, 64               # 6 x 512 x 512 x 64 x 2 B = 192 MiB exactly
    assert n * h * h * c * 2 == 192 << 20
    dy = torch.randn(n, 2 * h, 2 * h, c, device="cuda", dtype=dtype)
    act = torch.randn(n, h, h, c, device="cuda", dtype=dtype)
    outs = []
    for parts in ([(0, n)], [(0, n // 2), (n // 2, n)]):
        raw, masked = torch.zeros_like(act), torch.zeros_like(act)
        for lo, hi in parts:
            _assert_reaches(ROWS_BWD_NT if hi - lo == n else VECTOR[2], dtype, hi - lo, h, h, c, A.view(dy[lo:hi]), A.view(raw[lo:hi]), act=A.view(act[lo:hi]),
                            b2=A.view(masked[lo:hi]))
            A.check(L.srganfd_resample_bwd_lrelu(A.view(dy[lo:hi]), A.view(raw[lo:hi]), A.view(act[lo:hi]), A.view(masked[lo:hi]), A.F16, hi - lo, h, h, c, 0.2, st), "bwd_lrelu")
        torch.cuda.synchronize()
        outs.append((raw, masked))
    assert outs[0][0].float().abs().max() > 0 and not torch.equal(outs[0][0], outs[0][1])
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])


# ---- what is refused ----
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_refusals_write_nothing(dtype):
    A, L, st = O.abi()
    n, h, w, c = 2, 4, 6, 64
    dt = O.code(A, dtype)
    x = _randn((n, h, w, c), dtype, seed=9)
    sx, sy, sz = Slot((n, h, w, c), dtype, x, 32, 16), Slot((n, h, w, c), dtype, None, 32, 8), Slot((n, h, w, c), dtype, None, 32, 0)
    V = lambda s, **kw: A.view(s.buf, s.buf.shape[-1], kw.get("c0", s.c0), kw.get("planar", 0))
    bad = [
        lambda: L.srganfd_resample(4, V(sx, c0=40), V(sy), dt, n, h, w, c, st),            # c0 + c > cstride, either side
        lambda: L.srganfd_resample(4, V(sx), V(sy, c0=40), dt, n, h, w, c, st),
        lambda: L.srganfd_resample(5, V(sx), V(sy), dt, n, h, w, c, st),                   # no such op, vector and scalar dispatch
        lambda: L.srganfd_resample(-1, V(sx), V(sy), dt, n, h, w, c, st),
        lambda: L.srganfd_resample(5, V(sx, c0=2), V(sy, c0=2), dt, n, h, w, c, st),
        lambda: L.srganfd_resample(4, V(sx, planar=1), V(sy), dt, n, h, w, c, st),         # a planar view
        lambda: L.srganfd_resample(4, V(sx), V(sy, planar=1), dt, n, h, w, c, st),
        lambda: L.srganfd_resample_bwd_lrelu(V(sx), V(sy), V(sx), V(sz, planar=1), dt, n, h // 2, w // 2, c, 0.2, st),
        lambda: L.srganfd_resample_bwd_lrelu(V(sx), V(sy, c0=40), V(sx), V(sz), dt, n, h // 2, w // 2, c, 0.2, st),
        lambda: L.srganfd_resample_bwd_lrelu(V(sx), V(sy, c0=2), V(sx), V(sz), dt, n, h // 2, w // 2, c, 0.2, st),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(A.SrganfdError):
            A.check(f(), f"refusal {i}")
    torch.cuda.synchronize()
    for s in (sx, sy, sz):
        s.assert_untouched("refused call")
