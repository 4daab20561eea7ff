"""GPU parity of the individual HIP kernels (through the C ABI) against CPU torch ops.

f32 mode (v_mfma_f32_32x32x2_f32, exact fp32 fma chain): rel tolerance 2e-5.
bf16 / f16 modes (v_mfma_f32_32x32x16_bf16 / _f16, fp32 accumulate): the oracle is fed the SAME 16-bit-rounded
inputs/weights, so only accumulation order and the final 16-bit store differ: tolerance 1e-2 of the
output scale for bf16 (8 bits of mantissa -> 3.9e-3 per rounding), 1.5e-3 for f16 (11 bits -> 4.9e-4).
"""
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _tol(dtype):
    # f16 (v_mfma_f32_32x32x16_f16): 11 significant bits -> 4.9e-4 per rounding of the stored result
    return {torch.float32: 2e-5, torch.bfloat16: 1e-2, torch.float16: 1.5e-3}[dtype]


def _rt(t, dtype):
    """round-trip through the storage dtype (what the kernel sees)"""
    return t.to(dtype).to(torch.float64)


def _assert_close(got, want, dtype, what):
    got = got.detach().double().cpu()
    want = want.detach().double().cpu()
    scale = want.abs().max().item() + 1e-30
    err = (got - want).abs().max().item() / scale
    assert err < _tol(dtype), f"{what}: max err / scale = {err:.3e} (scale {scale:.3e})"


def _nhwc(t, dtype, cbuf=None, c0=0):
    """NCHW cpu tensor -> NHWC cuda buffer with cbuf channels, data at [c0, c0+C)"""
    n, c, h, w = t.shape
    cbuf = cbuf or c
    buf = torch.randn(n, h, w, cbuf) * 3.0  # garbage outside the view: must not be read
    buf[..., c0:c0 + c] = t.permute(0, 2, 3, 1)
    return buf.to(dtype).cuda()


# The product library runs the 16-bit kernels on v_mfma_f32_16x16x32 only (level 3).  An experiment build selected with SRGANFD_LIB
# (-DSRGANFD_EXPERIMENT: tools/build_variant.sh) also carries the 32x32x16 instantiations and the level switch: test both there.
_LEVELS = [0, 3] if os.environ.get("SRGANFD_LIB") else [3]


@pytest.fixture(params=_LEVELS, ids=["mfma32x32x16", "mfma16x16x32"][-len(_LEVELS):])
def mfma16(request):
    """MFMA form of the 16-bit kernels (weights are packed under the same setting)"""
    from sr_gan_fd_amd import _abi as A
    if hasattr(A.lib(), "srganfd_set_mfma16"):
        A.lib().srganfd_set_mfma16(request.param)
    assert A.lib().srganfd_get_mfma16() == request.param
    yield request.param
    if hasattr(A.lib(), "srganfd_set_mfma16"):
        A.lib().srganfd_set_mfma16(3)          # the library default


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [
    dict(n=2, h=16, w=16, cin=64, cout=32, act=1, bias=True),
    dict(n=1, h=12, w=20, cin=96, cout=32, act=1, bias=True),               # ragged tile edges
    dict(n=1, h=9, w=37, cin=192, cout=64, res=True, bias=True),            # conv5 + 2 residuals
    dict(n=1, h=8, w=8, cin=64, cout=64, up=1, act=1, bias=True),           # nearest x2 fused
    dict(n=1, h=16, w=16, cin=64, cout=3, bias=True, y_f32=True),           # padded cout, fp32 out
    dict(n=1, h=16, w=16, cin=3, cout=64, bias=True),                       # padded cin
    dict(n=1, h=16, w=24, cin=64, cout=128, k=4, s=2, act=1),               # discriminator down block
    dict(n=1, h=8, w=8, cin=512, cout=256, act=1),                          # wide channels
    dict(n=1, h=8, w=8, cin=64, cout=32, k=1, p=0, bias=True),              # 1x1
    dict(n=1, h=16, w=16, cin=64, cout=32, mask=True),                      # LeakyReLU' mask epilogue
])
def test_conv2d_forward(dtype, case, mfma16):
    from sr_gan_fd_amd import _abi as A, ops
    torch.manual_seed(1)
    dt = ops.DT[dtype]
    n, h, w, cin, cout = case["n"], case["h"], case["w"], case["cin"], case["cout"]
    k, s, p, up = case.get("k", 3), case.get("s", 1), case.get("p", 1), case.get("up", 0)
    x = torch.randn(n, cin, h, w)
    wt = torch.randn(cout, cin, k, k) / (cin * k * k) ** 0.5
    b = torch.randn(cout) if case.get("bias") else None
    cin_p, cout_p = ops.pad32(cin), ops.pad32(cout)
    xin = torch.zeros(n, cin_p, h, w); xin[:, :cin] = x
    xbuf = _nhwc(xin, dtype, cbuf=cin_p + 32, c0=32)
    wp = ops.pack_single(wt.cuda(), dt)
    hl, wl = h << up, w << up
    ho, wo = (hl + 2 * p - k) // s + 1, (wl + 2 * p - k) // s + 1
    ybuf_c, y_c0 = 96 if cout <= 64 else cout + 32, 32
    y_f32 = case.get("y_f32", False)
    ybuf = torch.full((n, ho, wo, ybuf_c), 7.0, dtype=torch.float32 if y_f32 else dtype, device="cuda")
    kw = dict(ksize=k, stride=s, pad=p, up=up, cout_store=cout, act=case.get("act", 0), y_f32=y_f32,
              bias=b.cuda() if b is not None else None)
    ref_in = _rt(x, dtype)
    if up:
        ref_in = F.interpolate(ref_in, scale_factor=2, mode="nearest")
    ref = F.conv2d(ref_in, _rt(wt, dtype), b.double() if b is not None else None, stride=s, padding=p)
    if case.get("act") == 1:
        ref = F.leaky_relu(ref, 0.2)
    keep = []
    if case.get("res"):
        r1 = torch.randn(n, cout, ho, wo); r2 = torch.randn(n, cout, ho, wo)
        r1b, r2b = _nhwc(r1, dtype, cbuf=cout + 32, c0=32), _nhwc(r2, dtype)
        keep += [r1b, r2b]
        kw.update(post_scale=0.04, r1=A.view(r1b, c0=32), r1_scale=0.2, r2=A.view(r2b), r2_scale=1.0)
        ref = ref * 0.04 + 0.2 * _rt(r1, dtype) + _rt(r2, dtype)
    if case.get("mask"):
        m = torch.randn(n, cout, ho, wo)
        mb = _nhwc(m, dtype)
        keep.append(mb)
        kw.update(mask=A.view(mb), mask_slope=0.2)
        ref = ref * torch.where(_rt(m, dtype) > 0, 1.0, 0.2)
    args = ops.conv_args(dt, A.view(xbuf, c0=32), A.view(ybuf, c0=y_c0), wp, n, h, w, cin_p, cout_p, **kw)
    ops.conv2d(args)
    torch.cuda.synchronize()
    got = ybuf[..., y_c0:y_c0 + cout].permute(0, 3, 1, 2)
    _assert_close(got, ref, dtype, f"conv {case}")
    # nothing outside the output view may be touched
    assert torch.all(ybuf[..., :y_c0] == 7.0) and torch.all(ybuf[..., y_c0 + cout:] == 7.0)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("planar", [0, 1])
@pytest.mark.parametrize("case", [
    dict(cin=64, cout=32, act=1, bias=True, kind="E0"),                                   # growth conv: 16-bit transposed tile
    dict(cin=160, cout=32, act=1, bias=True, post_scale=0.5, alpha=1.5, kind="E0"),
    dict(cin=96, cout=32, mask=True, kind="E4"),                                          # its data-gradient twin
    dict(cin=192, cout=64, bias=True, r1=True, kind="E1"),                                # conv5
    dict(cin=192, cout=64, bias=True, r1=True, r2=True, kind="E3"),                       # conv5 at the end of an RRDB
    dict(cin=64, cout=64, act=1, bias=True, kind="E0"),                                   # tail / VGG convs
    dict(cin=64, cout=64, mask=True, kind="E4"),
])
def test_conv2d_compile_time_epilogue_kinds_are_bitwise_the_runtime_epilogue(dtype, planar, case):
    """The 3x3 stride-1 16-bit launches run with an epilogue fixed at compile time (conv_igemm_kernel's EK); a launch that also asks for
    y2 takes the run-time epilogue.  Same inputs through both: y must be identical bit for bit (ragged tile edges included), and the
    kernel label must show the kind."""
    from sr_gan_fd_amd import _abi as A, ops, profiling
    torch.manual_seed(11)
    dt = ops.DT[dtype]
    n, h, w, cin, cout = 2, 21, 45, case["cin"], case["cout"]
    x = (torch.randn(n, h, w, 192, device="cuda") * 0.7).to(dtype)
    wt = torch.randn(cout, cin, 3, 3, device="cuda") / (cin * 9) ** 0.5
    wp = ops.pack_single(wt, dt)
    b = torch.randn(cout, device="cuda") if case.get("bias") else None
    C_ = 96 if cout == 32 else 64
    c0 = 32 if cout == 32 else 0
    kw = dict(bias=b, act=case.get("act", 0), post_scale=case.get("post_scale", 1.0), alpha=case.get("alpha", 1.0))
    keep = []
    if case.get("r1"):
        r1 = torch.randn(n, h, w, C_, device="cuda").to(dtype); keep.append(r1)
        kw.update(r1=A.view(r1, c0=c0, planar=planar), r1_scale=0.2)
    if case.get("r2"):
        r2 = torch.randn(n, h, w, C_, device="cuda").to(dtype); keep.append(r2)
        kw.update(r2=A.view(r2, c0=c0, planar=planar), r2_scale=1.0)
    if case.get("mask"):
        m = torch.randn(n, h, w, C_, device="cuda").to(dtype); keep.append(m)
        kw.update(mask=A.view(m, c0=c0, planar=planar), mask_slope=0.2)
    ya = torch.full((n, h, w, C_), 7.0, dtype=dtype, device="cuda")
    yb = torch.full((n, h, w, C_), 7.0, dtype=dtype, device="cuda")
    y2 = torch.empty(n, h, w, C_, dtype=dtype, device="cuda")
    a = ops.conv_args(dt, A.view(x, planar=planar), A.view(ya, c0=c0, planar=planar), wp, n, h, w, cin, cout, **kw)
    bq = ops.conv_args(dt, A.view(x, planar=planar), A.view(yb, c0=c0, planar=planar), wp, n, h, w, cin, cout, y2=A.view(y2, c0=c0, planar=planar), **kw)
    assert profiling.conv_label(a).endswith("," + case["kind"] + ">"), profiling.conv_label(a)
    assert ",E" not in profiling.conv_label(bq)
    ops.conv2d(a); ops.conv2d(bq)
    torch.cuda.synchronize()
    assert torch.equal(ya.view(torch.int16), yb.view(torch.int16))
    assert torch.isfinite(ya.float()).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv2d_dgrad_orientation(dtype, mfma16):
    """weights packed with transposed=1 turn the same kernel into the data-gradient pass"""
    from sr_gan_fd_amd import _abi as A, ops
    torch.manual_seed(2)
    dt = ops.DT[dtype]
    n, h, w, cin, cout = 1, 12, 20, 96, 32
    x = torch.randn(n, cin, h, w, dtype=torch.float64, requires_grad=True)
    wt = torch.randn(cout, cin, 3, 3) / 30
    dy = torch.randn(n, cout, h, w)
    F.conv2d(x, _rt(wt, dtype), None, padding=1).backward(_rt(dy, dtype))
    wp = ops.pack_single(wt.cuda(), dt, transposed=True)
    dyb = _nhwc(dy, dtype)
    dxb = torch.zeros(n, h, w, cin, dtype=dtype, device="cuda")
    ops.conv2d(ops.conv_args(dt, A.view(dyb), A.view(dxb), wp, n, h, w, cout, cin))
    torch.cuda.synchronize()
    _assert_close(dxb.permute(0, 3, 1, 2), x.grad, dtype, "dgrad")


def _wg(k, s, p, cin, cout, **kw):
    """a weight-gradient case whose OUTPUT image is 9 x 35: rows and columns both ragged against the 8- (stride 1) or 4-row (stride 2)
    by 32-pixel tile"""
    return dict(n=1, h=9 * s, w=35 * s, cin=cin, cout=cout, k=k, s=s, p=p, **kw)


# One case per path of the plan's arithmetic (cin / cout are the padded channel counts the plan sees).  A 64-channel range that holds
# one 32-channel unit beside ranges that hold two ("mixed units") keeps a 16-bit launch off the loader waves: register staging.
_WGRAD_PATH_CASES = [
    _wg(3, 1, 1, 32, 32),      # x pitch 1 / dy pitch 1, loader waves
    _wg(3, 2, 1, 32, 32),      # dy pitch 1 (3x3 stride 2 never takes the loader waves)
    _wg(3, 2, 1, 64, 64),      # dy pitch 2
    _wg(3, 2, 1, 32, 96),      # mixed dy units
    _wg(4, 2, 1, 64, 32),      # dy pitch 1, loader waves
    _wg(4, 2, 1, 64, 96),      # mixed units: register staging in 16-bit
    _wg(2, 2, 0, 32, 32),      # dy pitch 1
    _wg(2, 2, 0, 64, 64),      # dy pitch 2
    _wg(2, 2, 0, 32, 96),      # mixed dy units
    _wg(1, 1, 0, 32, 32),      # pitches 1 / 1
    _wg(1, 1, 0, 64, 64),      # pitches 2 / 2
    _wg(1, 1, 0, 32, 64),      # pitches 1 / 2
    _wg(1, 1, 0, 96, 32),      # x pitch 2, mixed units
]
# Several tiles per workgroup (12 tiles at stride 1, 18 at stride 2): with one split a workgroup goes round the double buffer many
# times, with two each makes half the trips.  Per kernel shape one case with equal units everywhere (the loader waves, where the shape
# has them) and one with mixed units.
_WGRAD_MULTI_TILE_CASES = [
    dict(_wg(k, s, p, cin, cout), n=3, splits=splits)
    for k, s, p, cin, cout in [(3, 1, 1, 64, 64), (3, 1, 1, 96, 32), (3, 2, 1, 64, 64), (3, 2, 1, 32, 96), (4, 2, 1, 64, 32),
                               (4, 2, 1, 64, 96), (2, 2, 0, 64, 64), (2, 2, 0, 32, 96), (1, 1, 0, 64, 64), (1, 1, 0, 96, 32)]
    for splits in (1, 2)
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [
    dict(n=2, h=16, w=16, cin=64, cout=32),
    dict(n=1, h=10, w=37, cin=96, cout=32),
    dict(n=1, h=12, w=20, cin=160, cout=32),
    dict(n=2, h=8, w=40, cin=192, cout=64),
    dict(n=1, h=8, w=8, cin=64, cout=64, up=1),
    dict(n=1, h=16, w=16, cin=3, cout=64),
    dict(n=1, h=16, w=16, cin=64, cout=3),
    dict(n=1, h=16, w=24, cin=64, cout=128, k=4, s=2),
    dict(n=3, h=8, w=8, cin=256, cout=128, splits=3),
] + _WGRAD_PATH_CASES + _WGRAD_MULTI_TILE_CASES)
def test_conv2d_wgrad(dtype, case):
    from sr_gan_fd_amd import _abi as A, ops
    torch.manual_seed(3)
    dt = ops.DT[dtype]
    n, h, w, cin, cout = case["n"], case["h"], case["w"], case["cin"], case["cout"]
    k, s, p, up = case.get("k", 3), case.get("s", 1), case.get("p", 1), case.get("up", 0)
    x = torch.randn(n, cin, h, w)
    wt = torch.zeros(cout, cin, k, k, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    xin = _rt(x, dtype)
    if up:
        xin = F.interpolate(xin, scale_factor=2, mode="nearest")
    y = F.conv2d(xin, wt, b, stride=s, padding=p)
    dy = torch.randn_like(y).float()
    y.backward(_rt(dy, dtype))
    cin_p, cout_p = ops.pad32(cin), ops.pad32(cout)
    xpad = torch.zeros(n, cin_p, h, w); xpad[:, :cin] = x
    dypad = torch.zeros(n, cout_p, *dy.shape[2:]); dypad[:, :cout] = dy
    xb, dyb = _nhwc(xpad, dtype, cbuf=cin_p + 32, c0=32), _nhwc(dypad, dtype, cbuf=cout_p + 32, c0=0)
    grads = torch.full((cout * cin * k * k + cout + 8,), 5.0, device="cuda")
    plan = ops.WgradPlan("cuda", dt, n, h, w, cin_p, cout_p,
                         [dict(cin=cin_p, cout=cout_p, dw_off=8, db_off=8 + cout * cin * k * k, co_dst=cout, ci_dst=cin,
                               alpha=0.5)], ksize=k, stride=s, pad=p, up=up, splits=case.get("splits", 0))
    ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device="cuda")
    plan.run(A.view(xb, c0=32), A.view(dyb, c0=0), grads, ws)
    torch.cuda.synchronize()
    dw = grads[8:8 + cout * cin * k * k].view(cout, cin, k, k)
    db = grads[8 + cout * cin * k * k:]
    tol_dtype = dtype
    _assert_close(dw, 0.5 * wt.grad, tol_dtype, f"wgrad dW {case}")
    _assert_close(db, 0.5 * b.grad, tol_dtype, f"wgrad db {case}")
    assert torch.all(grads[:8] == 5.0)
    # run twice with beta=1 semantics covered in the dense-block test; determinism: bitwise equal
    g2 = torch.full_like(grads, 5.0)
    plan.run(A.view(xb, c0=32), A.view(dyb, c0=0), g2, ws)
    torch.cuda.synchronize()
    assert torch.equal(grads, g2), "wgrad must be bitwise reproducible"


@pytest.mark.parametrize("dtype", DTYPES)
def test_wgrad_dense_block_fused(dtype):
    """five convs of a dense block (shared x = concat buffer, shared dy = stacked gradients) in one launch"""
    from sr_gan_fd_amd import _abi as A, ops
    torch.manual_seed(4)
    dt = ops.DT[dtype]
    n, h, w = 1, 12, 36
    cat = torch.randn(n, 192, h, w)
    dyall = torch.randn(n, 192, h, w)  # [dY5(64) | dY4 | dY3 | dY2 | dY1]
    convs, refs, off = [], [], 0
    lo = {5: 0, 4: 64, 3: 96, 2: 128, 1: 160}
    for kk in (1, 2, 3, 4, 5):
        cin, cout = 64 + 32 * (kk - 1), (64 if kk == 5 else 32)
        wt = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
        b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(_rt(cat[:, :cin], dtype), wt, b, padding=1)
        y.backward(_rt(dyall[:, lo[kk]:lo[kk] + cout], dtype))
        convs.append(dict(ci_lo=0, cin=cin, co_lo=lo[kk], cout=cout, dw_off=off, db_off=off + wt.numel(),
                          co_dst=cout, ci_dst=cin, beta=1.0))
        refs.append((off, wt.grad, b.grad))
        off += wt.numel() + cout
    grads = torch.ones(off, device="cuda")
    plan = ops.WgradPlan("cuda", dt, n, h, w, 192, 192, convs)
    ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device="cuda")
    catb, dyb = _nhwc(cat, dtype), _nhwc(dyall, dtype)  # keep alive: views hold raw pointers
    plan.run(A.view(catb), A.view(dyb), grads, ws)
    torch.cuda.synchronize()
    for o, gw, gb in refs:
        _assert_close(grads[o:o + gw.numel()].view_as(gw) - 1.0, gw, dtype, "fused dW")
        _assert_close(grads[o + gw.numel():o + gw.numel() + gb.numel()] - 1.0, gb, dtype, "fused db")


def test_clamp_grad_rgb_fast_path_matches_definition():
    """d pre = d sr where 0 <= pre <= 1 else 0, NCHW fp32 -> NHWC bf16 padded to 32 channels: the per-pixel vectorised kernel the
    generator's backward starts with (3 channels, 4-channel fp32 pre-clamp pixels) against the definition, incl. the zero padding"""
    from sr_gan_fd_amd import _abi as A
    torch.manual_seed(0)
    n, c, h, w = 3, 3, 37, 29
    dsr = torch.randn(n, c, h, w, device="cuda")
    pre = torch.randn(n, h, w, 4, device="cuda") * 0.8 + 0.5          # fp32 NHWC, pitch 4 (channel 3 unused)
    pre[0, 0, 0, 0], pre[0, 0, 1, 1] = 0.0, 1.0                       # the closed interval's ends pass the gradient
    dst = torch.full((n, h, w, 32), 7.0, device="cuda", dtype=torch.bfloat16)
    A.check(A.lib().srganfd_clamp_grad_to_nhwc(dsr.data_ptr(), A.view(pre), n, c, h, w, A.view(dst), A.BF16, 32, A.stream_ptr()), "clamp_grad")
    inside = (pre[..., :3] >= 0) & (pre[..., :3] <= 1)
    want = torch.where(inside, dsr.permute(0, 2, 3, 1), torch.zeros((), device="cuda")).bfloat16()
    assert torch.equal(dst[..., :3], want) and float(dst[..., 3:].abs().max()) == 0.0
    # the generic kernel (any pitch / padding) agrees: same call with a 16-channel padding takes it
    dst16 = torch.full((n, h, w, 16), 7.0, device="cuda", dtype=torch.bfloat16)
    A.check(A.lib().srganfd_clamp_grad_to_nhwc(dsr.data_ptr(), A.view(pre), n, c, h, w, A.view(dst16), A.BF16, 16, A.stream_ptr()), "clamp_grad")
    assert torch.equal(dst16[..., :3], want) and float(dst16[..., 3:].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_resample_bwd_lrelu_equals_two_passes(dtype):
    """srganfd_resample_bwd_lrelu (adjoint of bilinear x2 + LeakyReLU' of the upsampled layer, U-Net decoder backward,
    model.py:150-161): the raw output equals srganfd_resample(op 2) bit for bit; the masked output equals raw * mask in f32 and is one
    16-bit rounding away from the two-pass result otherwise (the fused kernel masks the fp32 value before rounding)."""
    from sr_gan_fd_amd import _abi as A, ops
    torch.manual_seed(4)
    n, h, w, c = 2, 9, 13, 64
    dtc = ops.DT[dtype]
    dy = torch.randn(n, 2 * h, 2 * w, c, device="cuda").to(dtype)
    act = torch.randn(n, h, w, c, device="cuda").to(dtype)
    raw, masked, two = (torch.empty(n, h, w, c, device="cuda", dtype=dtype) for _ in range(3))
    ref_raw = torch.empty_like(raw)
    L, st = A.lib(), A.stream_ptr()
    A.check(L.srganfd_resample(2, A.view(dy), A.view(ref_raw), dtc, n, h, w, c, st))
    A.check(L.srganfd_lrelu_bwd(A.view(ref_raw), A.view(act), A.NULL_VIEW, A.view(two), dtc, n * h * w, c, 0.2, st))
    A.check(L.srganfd_resample_bwd_lrelu(A.view(dy), A.view(raw), A.view(act), A.view(masked), dtc, n, h, w, c, 0.2, st))
    only = torch.empty_like(masked)
    A.check(L.srganfd_resample_bwd_lrelu(A.view(dy), A.NULL_VIEW, A.view(act), A.view(only), dtc, n, h, w, c, 0.2, st))
    torch.cuda.synchronize()
    assert torch.equal(raw, ref_raw) and torch.equal(only, masked)
    # against torch: the adjoint of F.interpolate(scale_factor=2, mode="bilinear")
    u = torch.zeros(n, c, h, w, device="cuda", requires_grad=True)
    F.interpolate(u, scale_factor=2, mode="bilinear", align_corners=False).backward(dy.float().permute(0, 3, 1, 2))
    want = u.grad.permute(0, 2, 3, 1) * torch.where(act.float() > 0, 1.0, 0.2)
    tol = 1e-6 if dtype == torch.float32 else (1e-2 if dtype == torch.bfloat16 else 1.5e-3)
    scale = want.abs().max().item()
    assert (masked.float() - want).abs().max().item() < tol * scale
    if dtype == torch.float32:
        assert torch.equal(masked, two)
    else:
        assert (masked.float() - two.float()).abs().max().item() < tol * scale


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_wgrad_partial_plus_batched_reduction_equals_fused_call(dtype):
    """srganfd_conv2d_wgrad_partial + srganfd_wgrad_reduce_batch (several launches' slabs reduced by one kernel: the generator's
    dense blocks) give bit for bit what srganfd_conv2d_wgrad gives per launch."""
    import ctypes as C
    from sr_gan_fd_amd import _abi as A, ops
    torch.manual_seed(6)
    dtc = ops.DT[dtype]
    n, h, w, cx, cy = 2, 24, 40, 64, 64
    convs = [dict(cin=64, cout=32, co_lo=32, dw_off=0, db_off=32 * 64 * 9, co_dst=32, ci_dst=64),
             dict(cin=32, cout=32, co_lo=0, dw_off=32 * 64 * 9 + 32, db_off=-1, co_dst=32, ci_dst=32)]
    total = 32 * 64 * 9 + 32 + 32 * 32 * 9
    plan = ops.WgradPlan(torch.device("cuda"), dtc, n, h, w, cx, cy, convs)
    L, st = A.lib(), A.stream_ptr()
    inputs = [((torch.randn(n, h, w, cx, device="cuda") * 0.5).to(dtype), (torch.randn(n, h, w, cy, device="cuda") * 0.1).to(dtype)) for _ in range(3)]
    fused, batched = [], []
    ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device="cuda")
    for x, dy in inputs:
        g = torch.full((total,), 7.0, device="cuda")
        plan.run(A.view(x), A.view(dy), g, ws)
        fused.append(g)
    wss = [torch.empty(plan.workspace_bytes, dtype=torch.uint8, device="cuda") for _ in inputs]
    jobs = (A.WgradReduceJob * len(inputs))()
    for j, (x, dy), w_ in zip(jobs, inputs, wss):
        A.check(L.srganfd_conv2d_wgrad_partial(plan.host, plan.dev.data_ptr(), A.view(x), A.view(dy), w_.data_ptr(), w_.numel(), st))
        g = torch.full((total,), 7.0, device="cuda")
        batched.append(g)
        j.plan_host, j.plan_dev, j.grads, j.scalars, j.workspace = C.addressof(plan.host), plan.dev.data_ptr(), g.data_ptr(), None, w_.data_ptr()
    A.check(L.srganfd_wgrad_reduce_batch(jobs, len(inputs), st))
    torch.cuda.synchronize()
    for a, b in zip(fused, batched):
        assert torch.equal(a, b) and a.abs().max().item() > 0
    with pytest.raises(A.SrganfdError):
        A.check(L.srganfd_wgrad_reduce_batch(jobs, 9, st))


def test_batched_spectral_norm_equals_per_layer_calls_and_torch():
    """srganfd_spectral_norm_batch / _grad_batch (all normalised layers of a discriminator in one group of launches) against the
    per-layer entry points -- bit for bit, including a list longer than one launch group and ragged shapes -- and the per-layer
    result against torch's own power iteration (torch/nn/utils/spectral_norm.py:62-114) at 1e-5."""
    import torch.nn.functional as F
    from sr_gan_fd_amd import _abi as A, ops
    L, st = A.lib(), A.stream_ptr()
    torch.manual_seed(5)
    shapes = [(128, 64 * 16), (256, 128 * 16), (512, 256 * 16), (256, 512 * 9), (128, 256 * 9), (64, 128 * 9), (64, 64 * 9), (64, 576),
              (33, 70), (1, 5), (96, 1)]                                     # 11 layers: two launch groups, ragged tails
    Ws = [torch.randn(r, c, device="cuda") for r, c in shapes]
    us = [F.normalize(torch.randn(r, device="cuda"), dim=0) for r, _ in shapes]
    vs = [F.normalize(torch.randn(c, device="cuda"), dim=0) for _, c in shapes]
    for training in (True, False):
        one = [(u.clone(), v.clone(), torch.zeros(2, device="cuda")) for u, v in zip(us, vs)]
        for W, (u, v, sg) in zip(Ws, one):
            ws = torch.empty(A.sn_ws_floats(*W.shape), device="cuda")
            A.check(L.srganfd_spectral_norm(W.data_ptr(), u.data_ptr(), v.data_ptr(), W.shape[0], W.shape[1], int(training), 1e-12,
                                            sg.data_ptr(), sg.data_ptr() + 4, ws.data_ptr(), st), "spectral_norm")
        bat = [(u.clone(), v.clone(), torch.zeros(2, device="cuda")) for u, v in zip(us, vs)]
        ws = torch.empty(sum(A.sn_ws_floats(*W.shape) for W in Ws), device="cuda")
        ops.spectral_norm_batch([(W.data_ptr(), u.data_ptr(), v.data_ptr(), W.shape[0], W.shape[1], sg.data_ptr(), sg.data_ptr() + 4)
                                 for W, (u, v, sg) in zip(Ws, bat)], training, ws)
        torch.cuda.synchronize()
        for W, a, b, u0, v0 in zip(Ws, one, bat, us, vs):
            assert all(torch.equal(x, y) for x, y in zip(a, b)), W.shape
            if training:
                v1 = F.normalize(torch.mv(W.t(), u0), dim=0, eps=1e-12)
                u1 = F.normalize(torch.mv(W, v1), dim=0, eps=1e-12)
            else:
                u1, v1 = u0, v0
            sigma = torch.dot(u1, torch.mv(W, v1))
            assert torch.allclose(a[0], u1, atol=1e-5) and torch.allclose(a[1], v1, atol=1e-5)
            assert abs(a[2][0].item() - sigma.item()) <= 1e-5 * max(1.0, abs(sigma.item())) and abs(a[2][1].item() * sigma.item() - 1) < 1e-5
    # gradient through W / sigma
    Gs = [torch.randn_like(W) for W in Ws]
    isg = [torch.tensor([1.0 / torch.dot(u, torch.mv(W, v)).item()], device="cuda") for W, u, v in zip(Ws, us, vs)]
    one = [torch.full_like(W, 7.0) for W in Ws]
    for W, G, u, v, i, d in zip(Ws, Gs, us, vs, isg, one):
        ws = torch.empty(A.SN_GRAD_WS_FLOATS, device="cuda")
        A.check(L.srganfd_spectral_norm_grad(G.data_ptr(), W.data_ptr(), u.data_ptr(), v.data_ptr(), i.data_ptr(), d.data_ptr(), W.shape[0], W.shape[1],
                                             0.0, ws.data_ptr(), st), "spectral_norm_grad")
    bat = [torch.full_like(W, 7.0) for W in Ws]
    ws = torch.empty(len(Ws) * A.SN_GRAD_WS_FLOATS, device="cuda")
    ops.spectral_norm_grad_batch([(G.data_ptr(), W.data_ptr(), u.data_ptr(), v.data_ptr(), i.data_ptr(), d.data_ptr(), W.shape[0], W.shape[1])
                                  for W, G, u, v, i, d in zip(Ws, Gs, us, vs, isg, bat)], ws)
    torch.cuda.synchronize()
    for W, G, u, v, i, a, b in zip(Ws, Gs, us, vs, isg, one, bat):
        assert torch.equal(a, b), W.shape
        Wl = W.clone().requires_grad_(True)
        ((Wl / torch.dot(u, torch.mv(Wl, v))) * G).sum().backward()
        assert (a - Wl.grad).abs().max().item() <= 1e-4 * Wl.grad.abs().max().item()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case", [
    dict(n=2, hd=8, wd=8, co=128, ci=64),                      # down_block1: one 64-channel block per class
    dict(n=1, hd=5, wd=19, co=256, ci=128, r1=True),           # two blocks per class, ragged tiles, skip gradient added
    dict(n=1, hd=6, wd=33, co=128, ci=256, mask=True),         # four blocks per class, LeakyReLU' mask
    dict(n=1, hd=7, wd=18, co=128, ci=64, form="k3s2", mask=True),   # A-ESRGAN encoder: 3x3 stride 2 pad 1 as 2x2-tap classes, one window
    dict(n=2, hd=6, wd=9, co=64, ci=96, form="k3s2"),                # ... 32-channel blocks (96 is not a multiple of 64): three of them -> refused
    dict(n=1, hd=9, wd=21, co=64, ci=64, form="k2s2", r1=True),      # attention gate theta: 2x2 stride 2 as 1x1 classes
])
def test_stride2_dgrad_four_classes_in_one_launch(dtype, case):
    """data gradient of a stride-2 conv (4x4 pad 1: model.py:103-114; A-ESRGAN's 3x3 pad 1 and 2x2 pad 0): the four output-parity classes
    as ONE launch (srganfd_conv_args.out_classes = 4) are bitwise the four single-class launches, and both are torch's gradient."""
    from sr_gan_fd_amd import _abi as A, ops
    torch.manual_seed(11)
    dt = ops.DT[dtype]
    form = case.get("form", "k4s2")
    kfull, pad, kcls, tbase, step = {"k4s2": (4, 1, 2, 2, 1), "k3s2": (3, 1, 2, 6, 0), "k2s2": (2, 0, 1, 10, 0)}[form]
    n, hd, wd, co, ci = case["n"], case["hd"], case["wd"], case["co"], case["ci"]
    H, W = 2 * hd, 2 * wd
    wt = torch.randn(co, ci, kfull, kfull) / 40
    dy = torch.randn(n, co, hd, wd)
    x = torch.zeros(n, ci, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, _rt(wt, dtype), None, stride=2, padding=pad).backward(_rt(dy, dtype))
    want = x.grad.clone()
    r1 = torch.randn(n, ci, H, W) if case.get("r1") else None
    mk = torch.randn(n, ci, H, W) if case.get("mask") else None
    if r1 is not None:
        want = want + _rt(r1, dtype)
    if mk is not None:
        want = want * torch.where(_rt(mk, dtype) > 0, 1.0, 0.2)
    pb = ops.packed_bytes(dt, kcls, co, ci)
    packed = torch.empty(4 * pb, dtype=torch.uint8, device="cuda")
    jobs = [ops.pack_job(c * pb, dt, kcls, co, ci, [dict(src_off=0, co_src=co, ci_src=ci, k_len=co, transposed=tbase + c)]) for c in range(4)]
    ops.PackTable(jobs, torch.device("cuda")).run(wt.cuda().contiguous(), packed)
    dyb = _nhwc(dy, dtype)
    r1b = _nhwc(r1, dtype) if r1 is not None else None
    mkb = _nhwc(mk, dtype) if mk is not None else None

    def run(classes):
        dxb = torch.full((n, H, W, ci), 7.0, dtype=dtype, device="cuda")
        for par in ([0] if classes == 4 else range(4)):
            py, px = par >> 1, par & 1
            a = ops.conv_args(dt, A.view(dyb), A.view(dxb), packed.data_ptr() + par * pb, n, hd, wd, co, ci, ksize=kcls, stride=1, pad=0,
                              r1=A.view(r1b) if r1b is not None else A.NULL_VIEW, r1_scale=1.0 if r1b is not None else 0.0,
                              mask=A.view(mkb) if mkb is not None else A.NULL_VIEW, mask_slope=0.2)
            a.h_out, a.w_out = hd, wd
            a.out_sy, a.out_sx, a.out_oy, a.out_ox = 2, 2, py, px
            a.out_h_full, a.out_w_full = H, W
            base = 1 if form == "k4s2" else 0
            a.pad_y, a.pad_x = (base, base) if classes == 4 else (base - py * step, base - px * step)
            a.out_classes, a.class_pad_step = classes, step
            ops.conv2d(a)
        torch.cuda.synchronize()
        return dxb

    four = run(0)
    _assert_close(four.permute(0, 3, 1, 2), want, dtype, "stride-2 dgrad, four class launches")
    ok = ops.class4_ok(dt, ci, [c * pb for c in range(4)], pb, ksize=kcls)
    assert ok == (ci != 96)                    # three 32-channel blocks per class: the class index is not a shift of the block index
    if ok:
        one = run(4)
        assert torch.equal(four, one)
    else:
        with pytest.raises(A.SrganfdError):
            run(4)
    # what the class launch is not: fp32 parity mode, other kernel shapes
    a = ops.conv_args(dt, A.view(dyb), A.view(four), packed.data_ptr(), n, hd, wd, co, ci)
    a.out_classes = 4
    with pytest.raises(A.SrganfdError):
        ops.conv2d(a)


@pytest.mark.parametrize("kind", ["kind0", "kind4", "runtime_y2"])
def test_conv2d_nontemporal_twin_is_bitwise_the_plain_kernel(kind):
    """Outputs beyond 192 MB leave the wide 3x3 kernels through non-temporal stores (a compile-time twin of kinds 0 / 4 / run-time):
    the same launch as two half batches (each below the threshold, plain stores) gives the same bits."""
    from sr_gan_fd_amd import _abi as A, ops
    torch.manual_seed(5)
    dt, dtype = A.F16, torch.float16
    n, h, c = 6, 512, 64                                        # 6 x 512 x 512 x 64 x 2 B = 201 MB
    x = torch.randn(n, h, h, c, device="cuda", dtype=dtype)
    wt = torch.randn(c, c, 3, 3, device="cuda") / 24
    wp = ops.pack_single(wt, dt)
    bias = torch.randn(c, device="cuda") if kind == "kind0" else None
    mask = torch.randn(n, h, h, c, device="cuda", dtype=dtype) if kind == "kind4" else None

    def run(lo, hi, y, y2):
        kw = dict(bias=bias, act=A.ACT_LRELU if kind == "kind0" else A.ACT_NONE)
        if mask is not None:
            kw.update(mask=A.view(mask[lo:hi]), mask_slope=0.2)
        if y2 is not None:
            kw.update(y2=A.view(y2[lo:hi]), r1=A.view(x[lo:hi]), r1_scale=1.0)
        ops.conv2d(ops.conv_args(dt, A.view(x[lo:hi]), A.view(y[lo:hi]), wp, hi - lo, h, h, c, c, **kw))

    outs = []
    for parts in ([(0, n)], [(0, n // 2), (n // 2, n)]):
        y = torch.zeros_like(x)
        y2 = torch.zeros_like(x) if kind == "runtime_y2" else None
        for lo, hi in parts:
            run(lo, hi, y, y2)
        torch.cuda.synchronize()
        outs.append((y, y2))
    assert outs[0][0].float().abs().max() > 0
    assert torch.equal(outs[0][0], outs[1][0])
    if kind == "runtime_y2":
        assert torch.equal(outs[0][1], outs[1][1])
