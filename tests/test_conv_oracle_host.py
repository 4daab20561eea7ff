"""tests/conv_oracle.py is itself checked (no GPU): the formula against independent torch compositions and autograd, the buffer helpers,
the criterion against an fp32 emulation -- and the case tables of tests/test_conv_paths_gpu.py against dispatch_conv: the launches they
build, asked for their kernel label with dummy pointers (srganfd_conv2d_describe launches nothing), must reach every instantiation of
conv_igemm_kernel and no other."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_oracle as O
from tests import test_conv_paths_gpu as P

F64 = torch.float64


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _factor(m, slope):
    """1 where m > 0, else slope, in float64 (torch.where on two Python scalars gives fp32)"""
    return torch.where(m > 0, torch.ones_like(m), torch.full_like(m, slope))


@pytest.mark.parametrize("k,s,p,up", [(3, 1, 1, 0), (3, 1, 1, 1), (3, 2, 1, 0), (4, 2, 1, 0), (2, 2, 0, 0), (2, 1, 1, 0), (1, 1, 0, 0), (4, 2, 1, 1)])
@pytest.mark.parametrize("act", [O.ACT_NONE, O.ACT_LRELU, O.ACT_RELU])
def test_formula_against_torch_composition(k, s, p, up, act):
    torch.manual_seed(k * 100 + s * 10 + up + act)
    n, h, w, ci, co = 2, 9, 11, 5, 7
    x, wt, b = torch.randn(n, h, w, ci, dtype=F64), torch.randn(co, ci, k, k, dtype=F64), torch.randn(co, dtype=F64)
    xin = _nchw(x)
    if up:
        xin = F.interpolate(xin, scale_factor=2, mode="nearest")
    c = F.conv2d(xin, wt, None, stride=s, padding=p)
    r1, r2, m = (torch.randn(n, c.shape[2], c.shape[3], co, dtype=F64) for _ in range(3))
    adev = torch.tensor([0.6], dtype=torch.float32)
    v = 1.5 * float(adev.double()) * c + b.view(1, -1, 1, 1)
    v = {O.ACT_NONE: v, O.ACT_LRELU: F.leaky_relu(v, 0.1), O.ACT_RELU: F.relu(v)}[act]
    want2 = 0.5 * v
    want = (want2 + 0.2 * _nchw(r1) - 1.25 * _nchw(r2)) * _factor(_nchw(m), 0.3)
    y, y2, A = O.conv2d(x, wt, stride=s, pad=p, up=up, alpha=1.5, alpha_dev=adev, bias=b, act=act, slope=0.1, post_scale=0.5,
                        r1=r1, r1_scale=0.2, r2=r2, r2_scale=-1.25, mask=m, mask_slope=0.3)
    assert torch.allclose(y, _nhwc(want), rtol=1e-12, atol=1e-12)
    # y2 is the value BEFORE the residual adds and the mask
    assert torch.allclose(y2, _nhwc(want2), rtol=1e-12, atol=1e-12)
    assert not torch.allclose(y2, y)
    # A: the same on absolute values, activation and mask as factor 1
    wantA = 0.5 * (0.9 * F.conv2d(xin.abs(), wt.abs(), None, stride=s, padding=p) + b.abs().view(1, -1, 1, 1)) + 0.2 * _nchw(r1).abs() + 1.25 * _nchw(r2).abs()
    assert torch.allclose(A, _nhwc(wantA), rtol=1e-6) and bool((A >= y.abs() * (1 - 1e-12)).all())
    # cout_store: the first channels
    ys, y2s, As = O.conv2d(x, wt, stride=s, pad=p, up=up, alpha=1.5, alpha_dev=adev, bias=b[:3], act=act, slope=0.1, post_scale=0.5,
                           r1=r1, r1_scale=0.2, r2=r2, r2_scale=-1.25, mask=m, mask_slope=0.3, cout_store=3)
    assert torch.equal(ys, y[..., :3]) and torch.equal(y2s, y2[..., :3]) and torch.equal(As, A[..., :3])


def test_dgrad_orientation_is_autograd_of_conv2d():
    torch.manual_seed(2)
    n, h, w, ci, co = 2, 7, 10, 6, 4
    x = torch.zeros(n, ci, h, w, dtype=F64, requires_grad=True)
    wt, dy = torch.randn(co, ci, 3, 3, dtype=F64), torch.randn(n, h, w, co, dtype=F64)
    F.conv2d(x, wt, None, padding=1).backward(_nchw(dy))
    y, _, _ = O.conv2d(dy, O.weight_dgrad(wt), stride=1, pad=1)
    assert torch.allclose(y, _nhwc(x.grad), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("form", ["k4s2", "k3s2", "k2s2"])
def test_four_class_form_is_autograd_of_the_stride2_conv(form):
    """each class on its own (a strided single-class output with the full-image r1 / mask) and all four together"""
    torch.manual_seed(3)
    kf, pad, kc, _, _, _ = O.CLASS_FORMS[form]
    n, hd, wd, co, ci = 2, 5, 7, 6, 4
    x = torch.zeros(n, ci, 2 * hd, 2 * wd, dtype=F64, requires_grad=True)
    wt, dy = torch.randn(co, ci, kf, kf, dtype=F64), torch.randn(n, hd, wd, co, dtype=F64)
    out = F.conv2d(x, wt, None, stride=2, padding=pad)
    assert out.shape[2:] == (hd, wd)
    out.backward(_nchw(dy))
    r1, m = torch.randn(n, 2 * hd, 2 * wd, ci, dtype=F64), torch.randn(n, 2 * hd, 2 * wd, ci, dtype=F64)
    want = (_nhwc(x.grad) + r1) * _factor(m, 0.2)
    ws = [O.weight_class(wt, form, par) for par in range(4)]
    assert all(tuple(wc.shape) == (ci, co, kc, kc) for wc in ws)
    y, y2, _ = O.conv2d_classes(dy, ws, form, r1=r1, r1_scale=1.0, mask=m, mask_slope=0.2)
    assert torch.allclose(y, want, rtol=1e-12, atol=1e-12)
    assert torch.allclose(y2, _nhwc(x.grad), rtol=1e-12, atol=1e-12)
    for par in range(4):
        yc, _, _ = O.conv2d(dy, ws[par], stride=1, out=O.class_out(form, par, hd, wd), r1=r1, r1_scale=1.0, mask=m, mask_slope=0.2)
        assert torch.allclose(yc, want[:, (par >> 1)::2, (par & 1)::2], rtol=1e-12, atol=1e-12)


def test_planar_helpers_round_trip():
    torch.manual_seed(4)
    n, h, w, c = 2, 3, 5, 96
    t = torch.randn(n, h, w, c)
    p = O.to_planar(t)
    assert p.shape == (n, 3, h, w, 32) and p.is_contiguous()
    # srganfd_view.planar: element (pixel, channel) of an image at (c / 32) * H*W*32 + pixel * 32 + c % 32
    flat = p.reshape(n, -1)
    for (y, x, ch) in [(0, 0, 0), (2, 4, 95), (1, 3, 40)]:
        assert flat[1, (ch // 32) * h * w * 32 + (y * w + x) * 32 + ch % 32] == t[1, y, x, ch]
    assert torch.equal(O.from_planar(p), t)
    for planar in (0, 1):
        b = O.Buf(n, h, w, c, torch.bfloat16, planar, fill="garbage", gen=torch.Generator().manual_seed(0))
        b.put(32, t[..., :32])
        b.upload("cpu")
        got = b.download().clone()
        assert torch.equal(got, b.host) and torch.equal(got[..., 32:64], t[..., :32].bfloat16())
        b.assert_outside_untouched(got, 32, 32, "unchanged")
        got[0, 0, 0, 64] = 1.0
        with pytest.raises(AssertionError):
            b.assert_outside_untouched(got, 32, 32, "changed")
    s = O.Buf(1, 2, 2, 32, torch.float16)
    assert bool((s.host == O.SENTINEL).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("cin", [32, 192])
def test_criterion_holds_an_fp32_emulation_and_catches_one_zeroed_tap(dtype, cin):
    """the formula in fp32 arithmetic (torch's own fp32 conv: some other summation order), rounded once to the stored type, stays
    inside the bound (seen here at cin 32 / 192: 0.91 / 0.45 of it in bf16, 0.66 / 0.13 in f16 -- at cin 32 the rounding term is nearly
    used up, as it must be for a bound that is to notice a second rounding); with ONE weight tap of ONE input channel zeroed, 12 to
    91 % of the elements leave it"""
    torch.manual_seed(cin)
    n, h, w, co = 1, 12, 20, 32
    x = (torch.randn(n, h, w, cin) * 0.7).to(dtype)
    wt = (torch.randn(co, cin, 3, 3) / (cin * 9) ** 0.5).to(dtype)
    b = torch.randn(co)
    y, _, A = O.conv2d(x, wt, bias=b, act=O.ACT_LRELU, alpha=1.5, post_scale=0.5)

    def emulate(wq):
        v = 1.5 * F.conv2d(_nchw(x.float()), wq.float(), None, padding=1) + b.view(1, -1, 1, 1)
        return _nhwc(torch.where(v > 0, v * 0.5, v * (0.2 * 0.5))).to(dtype)

    ratio, _ = O.worst_ratio(emulate(wt), y, A, 9 * cin, dtype)
    wq = wt.clone()
    wq[:, 5, 1, 1] = 0
    bad = ((O.f64(emulate(wq)) - y).abs() > O.bound(y, A, 9 * cin, dtype)).double().mean().item()
    print(f"{dtype} cin {cin}: fp32 emulation at {ratio:.3f} of the bound; one tap zeroed: {100 * bad:.0f} % of the elements beyond it")
    assert ratio <= 1.0, ratio
    assert bad > 0.05, bad


# ---- path coverage: the labels the GPU cases reach, against the instantiations of dispatch_conv ----
_16 = ["KS=3,S=1,MR=2,WR=4,WN=2,M16,E0", "KS=3,S=1,MR=2,WR=4,WN=2,M16,E1", "KS=3,S=1,MR=2,WR=4,WN=2,M16,E3", "KS=3,S=1,MR=2,WR=4,WN=2,M16,E4",
       "KS=3,S=1,MR=2,WR=4,WN=2,M16", "KS=3,S=1,MR=2,WR=8,WN=1,M16,E0", "KS=3,S=1,MR=2,WR=8,WN=1,M16,E4", "KS=3,S=1,MR=2,WR=8,WN=1,M16",
       "KS=3,S=2,MR=1,WR=4,WN=2,M16", "KS=3,S=2,MR=1,WR=4,WN=1,M16", "KS=2,S=1,MR=2,WR=4,WN=2,M16", "KS=2,S=1,MR=2,WR=8,WN=1,M16",
       "KS=4,S=2,MR=1,WR=4,WN=2,M16,TS=2", "KS=4,S=2,MR=1,WR=4,WN=1,M16", "KS=2,S=2,MR=1,WR=4,WN=2,M16", "KS=2,S=2,MR=1,WR=4,WN=1,M16",
       "KS=1,S=1,MR=2,WR=4,WN=1,M16"]
_32 = ["KS=3,S=1,MR=2,WR=4,WN=2", "KS=3,S=1,MR=2,WR=8,WN=1", "KS=2,S=1,MR=2,WR=4,WN=2", "KS=2,S=1,MR=2,WR=8,WN=1", "KS=4,S=2,MR=1,WR=4,WN=1",
       "KS=3,S=2,MR=1,WR=4,WN=2", "KS=3,S=2,MR=1,WR=4,WN=1", "KS=2,S=2,MR=1,WR=4,WN=2", "KS=2,S=2,MR=1,WR=4,WN=1", "KS=1,S=1,MR=2,WR=4,WN=1"]
# the 44 instantiations dispatch_conv reaches below the non-temporal threshold: 17 per 16-bit type, 10 in f32
INSTANTIATIONS = {f"conv_igemm_kernel<{t},{s}>" for t in ("bf16", "f16") for s in _16} | {f"conv_igemm_kernel<f32,{s}>" for s in _32}
# class launches (out_classes = 4) the cases take: the same instantiations, marked by the label
CLASS_LABELS = {f"conv_igemm_kernel<{t},{s}>[4 classes]" for t in ("bf16", "f16")
                for s in ("KS=2,S=1,MR=2,WR=4,WN=2,M16", "KS=2,S=1,MR=2,WR=8,WN=1,M16", "KS=1,S=1,MR=2,WR=4,WN=1,M16")}
# the kernels that have a non-temporal twin (outputs of 192 MB and more): 4 per 16-bit type.  The label does not say which of the two
# a launch takes (launch_conv prints no NT), so what is held here is which kernels such shapes go to
NT_TWINS = {f"conv_igemm_kernel<{t},{s}" for t in ("bf16", "f16")
            for s in ("KS=3,S=1,MR=2,WR=4,WN=2,M16,E0>", "KS=3,S=1,MR=2,WR=4,WN=2,M16,E4>", "KS=3,S=1,MR=2,WR=4,WN=2,M16>", "KS=2,S=1,MR=2,WR=4,WN=2,M16>[4 classes]")}


def test_cases_reach_every_instantiation_and_no_other():
    from sr_gan_fd_amd import _abi as A, profiling
    assert len(INSTANTIATIONS) == 44 and len(NT_TWINS) == 8
    A.set_dry_run(True)
    try:
        seen = set()
        for case, dtype, cin, planar in P.SMALL_PARAMS:
            for a, lab, _ in P.dummy_launches(case, dtype, cin, planar):
                got = profiling.conv_label(a)
                assert got == lab, (case["name"], got, lab)
                seen.add(got)
        for case, dtype, planar in P.PERSISTENT_PARAMS:
            n, nblk, grid = P.persistent_batch(case, 256)
            for a, lab, _ in P.dummy_launches(case, dtype, case["cin"], planar, (n, P.PH, P.PW, P.PH, P.PW, case["cout"])):
                assert profiling.conv_label(a) == lab and lab.endswith(f",E{case['ek']}>")
                seen.add(lab)
        plain = {s for s in seen if not s.endswith("[4 classes]")}
        assert plain == INSTANTIATIONS, (sorted(INSTANTIATIONS - plain), sorted(plain - INSTANTIATIONS))
        assert seen - plain == CLASS_LABELS, sorted(seen - plain)
        # shapes of 192 MB of output and more: the kinds 0 / 4 / run-time of the wide 3x3 kernel and the wide 2x2 class launch with a bias
        nt = set()
        for dtype in P.HALF:
            big = (6, 512, 512, 512, 512, 64)                                  # 6 x 512 x 512 x 64 x 2 B = 201 MB
            assert big[0] * big[3] * big[4] * big[5] * 2 >= 192 << 20
            for extra in (dict(bias=True, act=O.ACT_LRELU, ek=0), dict(mask=0.2, ek=4), dict(r1=1.0, y2=True)):
                (a, lab, _), = P.dummy_launches(dict(P.DEFAULTS, name="big", **extra), dtype, 64, 0, big)
                assert profiling.conv_label(a) == lab
                nt.add(lab)
            cls = P.dummy_launches(dict(P.DEFAULTS, name="big_cls", form="k4s2", bias=True), dtype, 64, 0, (6, 256, 256, 512, 512, 64))
            a, lab, par = cls[-1]
            assert par == 4 and profiling.conv_label(a) == lab
            nt.add(lab)
        assert nt == NT_TWINS, sorted(nt ^ NT_TWINS)
    finally:
        A.set_dry_run(False)


@pytest.mark.parametrize("cus", [256, 304, 64])
def test_persistent_batches_meet_their_preconditions(cus):
    """the batch rule of the persistent cases on MI355X (256 compute units) and on other counts"""
    odd = 0
    for case in P.PERSISTENT:
        n, nblk, grid = P.persistent_batch(case, cus)
        assert nblk > 2 * cus and nblk > 2 * grid and nblk % grid != 0 and nblk < 3 * grid
        odd += nblk % 8 != 0
        if case.get("changes_block"):
            assert P.block_changes(case, nblk, grid), case["name"]
        elif cus == 256:
            # 1, 2 or 4 channel blocks and a grid of 512: every tile of a workgroup has the same channel block
            assert not P.block_changes(case, nblk, grid), case["name"]
    assert odd >= 1 and sum(bool(c.get("changes_block")) for c in P.PERSISTENT) >= 2


def test_case_tables_cover_what_they_promise():
    """both cin and every element type a path exists in; NHWC and planar wherever a launch may take planar views"""
    for c in P.SMALL:
        assert c["dtypes"] == P.ALL and (c["planar"] == (0, 1) or c["y_f32"] or c["y_c0"] == "unaligned"), c["name"]
    assert P.CINS == (32, 96)
    for c, dtype, cin, planar in P.SMALL_PARAMS:
        n, hi, wi, ho, wo, cout = P.geometry(c, dtype, cin)
        mr, wr, _ = (P.TILE32 if dtype == torch.float32 else P.TILE16)[((O.CLASS_FORMS[c["form"]][2], 1) if c["form"] else (c["k"], c["s"])) + (int(cout % 64 == 0),)]
        rows = hi if c["form"] else ho
        assert n == 2 and rows - c["up"] == 2 * mr * wr + 3 and (wi if c["form"] else wo) - c["up"] == 37
