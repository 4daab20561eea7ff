"""csrc/loss.hip, every launch line on its own against the float64 definitions of tests/step_oracle.py: the scalar losses with every flag
in both states, their gradients, the L1 loss and its gradient on channel-slice views, the non-finite flag at every position of its
vector body and scalar tail, and the device-resident loss scaler word for word.

Sizes follow the code: reductions run 256-thread blocks capped at 1024 (a second trip past 262 144 elements or chunks),
bce_rel_other_kernel caps at 256 blocks (65 536), l1_grad_views at 8192 (2 097 152), nonfinite_flag takes four elements per lane on
2048 blocks (a second quad per lane past 2 097 152 + 3).

Bounds (none measured on the code under test):
  a scalar loss            |got - ref| <= 1e-5 * |weight| * mean|term|, the mean over the absolute per-element terms: the two-stage sum
                           does about 20 fp32 roundings per path, about 1.2e-6 of that quantity (test_losses_match_torch holds 1e-5 too)
  sigmoid(mean x)          the same bound on the mean, 1e-5 * mean|x|, through a slope of at most 1/4, plus TOL_FWD of the result
  gradients                norm_oracle.assert_f32 / assert_stored at TOL_FWD
The workspace is fenced beyond SRGANFD_LOSS_WS_FLOATS, every output slot and gradient with 8 sentinels on either side.

NaN follows torch: a NaN input makes the loss NaN (through relu_first as well: torch.relu keeps a NaN, fmaxf did not).  The L1 gradients
at a NaN difference are 0, because torch.sign is (0 < d) - (d < 0) and gives 0 there, under autograd too (tests/test_step_host.py pins
it): the kernels already did that, and test_l1_loss_nan_is_torchs holds them to torch's gradient bit for bit.

Which test reaches which launch (SRGANFD_LAUNCH lines of csrc/loss.hip):
  l1_partial_kernel, finish_kernel<FinAxpy>              test_l1_loss, test_l1_loss_nan_is_torchs
  l1_views_partial_kernel<T, N> (vector and N = 1)       test_l1_loss_views, test_l1_loss_views_keeps_a_nan_through_relu,
                                                         test_l1_loss_views_one_view_off_the_vector_takes_the_scalar_form (N = 1)
  l1_grad_views_kernel                                   test_l1_grad_views, test_l1_grad_views_second_trip
  bce_partial_kernel, finish_kernel<FinAxpy> (both uses) test_bce_logits
  sum_partial_kernel, finish_kernel<FinSigmoidMean>      test_sigmoid_of_mean
  sum_partial_kernel, finish_kernel<FinMean>, bce_rel_partial_kernel, finish_kernel<FinAxpy>, bce_rel_other_kernel       test_bce_logits_relativistic
  nonfinite_flag_kernel                                  test_nonfinite_flag
  loss_scale_update_kernel                               test_loss_scale_update_word_for_word"""
import numpy as np
import pytest
import torch

from tests import step_oracle as O

pytestmark = pytest.mark.gpu

DTYPES, IDS, Slot, Fenced, SENTINEL = O.DTYPES, O.IDS, O.Slot, O.Fenced, O.SENTINEL
RED = 1024 * 256                                             # threads of a reduction's grid: one element more takes a second trip
SIZES = [1, 2, 16, 65, 257, RED, RED + 1, 2 * RED + 37]
LOSS_SCALE = 1024.0


def _gen(seed):
    return torch.Generator().manual_seed(seed)


class _Call:
    """what every loss call shares: the fenced workspace, the loss slot, the device-resident loss scale"""

    def __init__(self):
        self.A, self.L, self.st = O.abi()
        self.ws = Fenced(n=self.A.LOSS_WS_FLOATS)
        self.scale = torch.tensor([LOSS_SCALE], device="cuda")

    def slot(self, prev):
        return Fenced(torch.tensor([SENTINEL if prev is None else prev]))

    def done(self, what):
        torch.cuda.synchronize()
        self.ws.assert_fences(what + ": workspace")
        assert self.scale.item() == LOSS_SCALE


def _assert_loss(slot, prev, ref, weight, mean_abs_term, what):
    slot.assert_fences(what)
    got, want = slot.val.item(), (prev or 0.0) + float(ref)
    bound = 1e-5 * abs(weight) * float(mean_abs_term)
    print(f"{what}: {got!r} against {want!r}, off by {abs(got - want):.2e} (bound {bound:.2e})")
    assert np.isfinite(got) and abs(got - want) <= bound, what


def _assert_grad(f, ref, what, exact_zero=None):
    f.assert_fences(what)
    O.assert_f32(f.val, ref, O.TOL_FWD, what)
    if exact_zero is not None and exact_zero.any():
        assert (f.val.cpu()[exact_zero] == 0).all(), what + ": not 0 at a tie"


# (weight, accumulate onto, gradient asked for, grad_scale, through the device-resident scale)
FLAGS = [(20.0, None, True, 20.0, False), (0.5, 0.25, False, 0.5, False), (1.0, None, True, 3.0, True), (-2.0, -0.75, True, -2.0, True)]


# ---- L1 on flat arrays ----
@pytest.mark.parametrize("n", SIZES)
def test_l1_loss(n):
    k = _Call()
    a, b = torch.rand(n, generator=_gen(n)), torch.rand(n, generator=_gen(n + 1))
    tie = torch.zeros(n, dtype=torch.bool)
    if n >= 2:
        tie[[1, n - 1]] = True
        b[tie] = a[tie]
    fa, fb = Fenced(a), Fenced(b)
    mean_abs = (a.double() - b.double()).abs().mean()
    for weight, prev, want_grad, gs, dev in FLAGS:
        what = f"l1_loss n={n} weight={weight} accumulate={prev} grad={want_grad} scale_dev={dev}"
        out, grad = k.slot(prev), Fenced(n=n)
        k.A.check(k.L.srganfd_l1_loss(fa.ptr(), fb.ptr(), n, weight, out.ptr(), 0 if prev is None else 1, grad.ptr() if want_grad else None, gs,
                                      k.scale.data_ptr() if dev else None, k.ws.ptr(), k.st), what)
        k.done(what)
        fa.assert_untouched("a")
        fb.assert_untouched("b")
        loss, g = O.l1(a, b, O.f32(weight))
        _assert_loss(out, prev, loss, weight, mean_abs, what)
        if want_grad:
            _assert_grad(grad, g * (O.f32(gs) * (LOSS_SCALE if dev else 1.0) / O.f32(weight)), what, tie)
        else:
            grad.assert_untouched(what + ": a gradient nobody asked for")


def test_l1_loss_nan_is_torchs():
    """a NaN in a: the loss is NaN; the gradient is torch.sign's, 0 at the NaN and untouched by it elsewhere"""
    k = _Call()
    n = 1000
    a, b = torch.rand(n, generator=_gen(1)), torch.rand(n, generator=_gen(2))
    a[[0, 517, n - 1]] = float("nan")
    ar = a.clone().requires_grad_(True)
    ref = torch.nn.functional.l1_loss(ar, b)
    ref.backward()
    assert torch.isnan(ref) and (ar.grad[[0, 517, n - 1]] == 0).all()
    out, grad, fa, fb = k.slot(None), Fenced(n=n), Fenced(a), Fenced(b)
    k.A.check(k.L.srganfd_l1_loss(fa.ptr(), fb.ptr(), n, 1.0, out.ptr(), 0, grad.ptr(), 1.0, None, k.ws.ptr(), k.st), "l1_loss")
    k.done("l1_loss")
    out.assert_fences("loss")
    assert torch.isnan(out.val).all()
    _assert_grad(grad, O.l1(a, b)[1], "l1 gradient beside a NaN", torch.isnan(a))
    O.assert_bits(grad.val.cpu(), ar.grad, "l1 gradient against torch's")


# ---- L1 between channel-slice views ----
VIEW_CASES = [("vector", 64), ("scalar", 3)]


def _views_case(dtype, form, c, size, seed):
    v = O.vn(dtype)
    if size == "small":
        npix = 37 * 29
    else:                                                     # the chunk (vector form) or element (scalar form) count crosses 262 144 once
        npix = RED // (c // v) + 3 if form == "vector" else RED // c + 7
        assert RED < npix * (c // v if form == "vector" else c) < 2 * RED
    g = _gen(seed)
    a, b = torch.randn(npix, c, generator=g).to(dtype), torch.randn(npix, c, generator=g).to(dtype)
    geo = [(2 * v, v), (v, 0)] if form == "vector" else [(5, 2), (2, 1)]
    return a, b, geo


@pytest.mark.parametrize("size", ["small", "second trip"])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("form,c", VIEW_CASES, ids=[f for f, _ in VIEW_CASES])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_l1_loss_views(dtype, form, c, relu, size):
    k = _Call()
    a, b, geo = _views_case(dtype, form, c, size, seed=3 + relu)
    npix = a.shape[0]
    sa, sb = Slot((npix, c), dtype, a, *geo[0]), Slot((npix, c), dtype, b, *geo[1])
    ref = O.l1_views(a, b, bool(relu))
    for weight, prev in ((1.0, None), (0.1, 0.25)):
        what = f"l1_loss_views {form} relu={relu} weight={weight} accumulate={prev}"
        out = k.slot(prev)
        k.A.check(k.L.srganfd_l1_loss_views(sa.view(k.A), sb.view(k.A), O.code(k.A, dtype), npix, c, relu, weight, out.ptr(), 0 if prev is None else 1,
                                            k.ws.ptr(), k.st), what)
        k.done(what)
        sa.assert_untouched("a")
        sb.assert_untouched("b")
        _assert_loss(out, prev, O.f32(weight) * ref, weight, ref, what)


@pytest.mark.parametrize("form,c", VIEW_CASES, ids=[f for f, _ in VIEW_CASES])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_l1_loss_views_keeps_a_nan_through_relu(dtype, form, c):
    """torch.relu keeps a NaN, so F.l1_loss(relu(a), relu(b)) is NaN: the content loss must not stay finite over a NaN feature"""
    k = _Call()
    a, b, geo = _views_case(dtype, form, c, "small", seed=5)
    npix = a.shape[0]
    for where in ((0, 0), (npix - 1, c - 1)):
        for relu in (0, 1):
            an = a.clone()
            an[where] = float("nan")
            assert torch.isnan(O.l1_views(an, b, bool(relu)))
            out, sa, sb = k.slot(None), Slot((npix, c), dtype, an, *geo[0]), Slot((npix, c), dtype, b, *geo[1])
            k.A.check(k.L.srganfd_l1_loss_views(sa.view(k.A), sb.view(k.A), O.code(k.A, dtype),
                                                npix, c, relu, 1.0, out.ptr(), 0, k.ws.ptr(), k.st), "l1_loss_views")
            k.done("l1_loss_views")
            out.assert_fences("loss")
            assert torch.isnan(out.val).all(), f"NaN at {where}, relu={relu}: the loss is {out.val.item()}"


@pytest.mark.parametrize("how", ["c0 one channel off", "cstride off the vector"])
@pytest.mark.parametrize("which", [0, 1], ids=["a", "b"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_l1_loss_views_one_view_off_the_vector_takes_the_scalar_form(dtype, which, how):
    """c a multiple of the vector and the base pointers aligned; exactly one term of the eligibility test fails, for exactly one view.  The
    vector form would read that view's pixels at addresses that are no multiple of 16 bytes (the sum is the check: the two forms add in
    different orders, so they are not held to each other's bits)."""
    k = _Call()
    v = O.vn(dtype)
    npix, c = 37 * 29, 2 * v
    g = _gen(7)
    a, b = torch.randn(npix, c, generator=g).to(dtype), torch.randn(npix, c, generator=g).to(dtype)
    geo = [(2 * v, v), (v, 0)]
    pad, c0 = geo[which]
    geo[which] = (pad, c0 + 1) if how.startswith("c0") else (pad + 1, c0)
    sa, sb = Slot((npix, c), dtype, a, *geo[0]), Slot((npix, c), dtype, b, *geo[1])
    for relu in (0, 1):
        ref = O.l1_views(a, b, bool(relu))
        what = f"l1_loss_views, {'ab'[which]} {how}, relu={relu}"
        out = k.slot(0.25)
        k.A.check(k.L.srganfd_l1_loss_views(sa.view(k.A), sb.view(k.A), O.code(k.A, dtype), npix, c, relu, 0.1, out.ptr(), 1, k.ws.ptr(), k.st), what)
        k.done(what)
        sa.assert_untouched("a")
        sb.assert_untouched("b")
        _assert_loss(out, 0.25, O.f32(0.1) * ref, 0.1, ref, what)


def _l1_grad_views(dtype, npix, c, geo, upstream, seed, device="cpu"):
    A, L, st = O.abi()
    g = torch.Generator(device=device).manual_seed(seed)
    a, b = torch.randn(npix, c, generator=g, device=device).to(dtype), torch.randn(npix, c, generator=g, device=device).to(dtype)
    tie = torch.zeros(npix, c, dtype=torch.bool, device=device)
    tie[0, 0] = tie[npix // 2, c // 2] = tie[-1, -1] = True
    b[tie] = a[tie]
    sa, sb, so = Slot((npix, c), dtype, a, *geo[0]), Slot((npix, c), dtype, b, *geo[1]), Slot((npix + 1, c), dtype, None, *geo[2])
    up = torch.tensor([upstream], device="cuda") if upstream is not None else None
    scale = 20.0 / (npix * c)
    A.check(L.srganfd_l1_grad_views(sa.view(A), sb.view(A), so.view(A), O.code(A, dtype), npix, c, up.data_ptr() if up is not None else None, scale, st), "l1_grad_views")
    torch.cuda.synchronize()
    sa.assert_untouched("a")
    sb.assert_untouched("b")
    so.assert_outside_untouched("l1_grad_views")
    assert (so.val[npix] == SENTINEL).all(), "the pixel behind the last one was written"
    got = so.val[:npix]
    O.assert_stored(got, O.l1_grad_views(a, b, O.f32(scale), upstream), O.TOL_FWD, f"l1_grad_views upstream={upstream}")
    assert (got[tie.to(got.device)] == 0).all(), "not 0 at a tie"
    assert (got.float().abs().unique().numel()) == 2, "one magnitude and 0"


@pytest.mark.parametrize("upstream", [None, -LOSS_SCALE], ids=["no-upstream", "upstream"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_l1_grad_views(dtype, upstream):
    v = O.vn(dtype)
    _l1_grad_views(dtype, 37 * 29, 3 * v, [(2 * v, v), (v, 0), (v, v)], upstream, seed=6)
    _l1_grad_views(dtype, 37 * 29, 3, [(5, 2), (2, 1), (1, 0)], upstream, seed=7)


def test_l1_grad_views_second_trip():
    """8 x (262 144 + 5) = 2 097 192 elements on a grid capped at 2 097 152 threads; a tie in the last element"""
    _l1_grad_views(torch.float16, RED + 5, 8, [(0, 0), (8, 0), (8, 8)], LOSS_SCALE, seed=8, device="cuda")


# ---- BCE with logits ----
def _logits(n, seed, scale=3.0):
    x = torch.randn(n, generator=_gen(seed)) * scale
    if n >= 16:
        x[[0, n - 1]] = 90.0
        x[[1, n - 2]] = -90.0
        x[2] = 0.0
    return x


@pytest.mark.parametrize("target", [0.0, 1.0])
@pytest.mark.parametrize("n", SIZES)
def test_bce_logits(n, target):
    k = _Call()
    x = _logits(n, n)
    fx = Fenced(x)
    loss, sig, g = O.bce(x, target)
    for i, (weight, prev, want_grad, gs, dev) in enumerate(FLAGS):
        what = f"bce_logits n={n} target={target} weight={weight} accumulate={prev} grad={want_grad} scale_dev={dev}"
        want_sig = i % 2 == 0
        out, sm, grad = k.slot(prev), k.slot(None), Fenced(n=n)
        k.A.check(k.L.srganfd_bce_logits(fx.ptr(), n, target, weight, out.ptr(), 0 if prev is None else 1, sm.ptr() if want_sig else None,
                                         grad.ptr() if want_grad else None, gs, k.scale.data_ptr() if dev else None, k.ws.ptr(), k.st), what)
        k.done(what)
        fx.assert_untouched("logits")
        _assert_loss(out, prev, O.f32(weight) * loss, weight, loss, what)
        if want_sig:
            _assert_loss(sm, None, sig, 1.0, sig, what + ": mean sigmoid")
        else:
            sm.assert_untouched(what + ": a sigmoid mean nobody asked for")
        if want_grad:
            _assert_grad(grad, g * (O.f32(gs) * (LOSS_SCALE if dev else 1.0)), what)
        else:
            grad.assert_untouched(what + ": a gradient nobody asked for")


@pytest.mark.parametrize("n", SIZES)
def test_sigmoid_of_mean(n):
    k = _Call()
    for shift in (0.0, 2.5):
        x = _logits(n, 100 + n) + shift
        fx, out = Fenced(x), k.slot(None)
        k.A.check(k.L.srganfd_sigmoid_of_mean(fx.ptr(), n, out.ptr(), k.ws.ptr(), k.st), "sigmoid_of_mean")
        k.done("sigmoid_of_mean")
        fx.assert_untouched("logits")
        out.assert_fences("sigmoid_of_mean")
        ref = O.sigmoid_of_mean(x).item()
        bound = 1e-5 * x.double().abs().mean().item() / 4 + O.TOL_FWD * ref
        print(f"sigmoid_of_mean n={n}: {out.val.item()!r} against {ref!r} (bound {bound:.2e})")
        assert abs(out.val.item() - ref) <= bound


# ---- relativistic-average BCE ----
REL_SIZES = [(n, n) for n in SIZES] + [(16, 5), (5, 16), (257, 65536 + 3), (RED + 1, 65)]
# (target, weight, accumulate onto, grad_x: None / "set" / "add", grad_other likewise, grad_scale, through the device-resident scale)
REL_FLAGS = [(1.0, 1.0, None, "set", "set", 1.0, False), (0.0, 0.005, 0.002, "add", "add", 0.005, True), (1.0, -2.0, None, None, "set", 0.5, False),
             (0.0, 1.0, -0.75, "set", None, 1.0, True), (1.0, 0.5, None, "add", "set", 0.5, False), (0.0, 0.5, None, "set", "add", 0.5, False)]


@pytest.mark.parametrize("n,n_other", REL_SIZES)
def test_bce_logits_relativistic(n, n_other):
    k = _Call()
    x, other = _logits(n, 200 + n), _logits(n_other, 300 + n_other) + 0.5
    fx, fo = Fenced(x), Fenced(other)
    for target, weight, prev, gx_mode, go_mode, gs, dev in REL_FLAGS:
        what = f"bce_relativistic n={n} n_other={n_other} target={target} weight={weight} accumulate={prev} grad_x={gx_mode} grad_other={go_mode} scale_dev={dev}"
        loss, gx, go = O.bce_relativistic(x, other, target)
        s = O.f32(gs) * (LOSS_SCALE if dev else 1.0)
        # what an accumulating call finds in the buffer: of the size of what it adds, so that neither hides the other
        gx0 = torch.randn(n, generator=_gen(1)) * abs(s) / n
        go0 = torch.randn(n_other, generator=_gen(2)) * abs(s) / n_other
        out = k.slot(prev)
        fgx = Fenced(gx0) if gx_mode == "add" else Fenced(n=n)
        fgo = Fenced(go0) if go_mode == "add" else Fenced(n=n_other)
        k.A.check(k.L.srganfd_bce_logits_relativistic(fx.ptr(), n, fo.ptr(), n_other, target, weight, out.ptr(), 0 if prev is None else 1,
                                                      fgx.ptr() if gx_mode else None, 1 if gx_mode == "add" else 0,
                                                      fgo.ptr() if go_mode else None, 1 if go_mode == "add" else 0, gs,
                                                      k.scale.data_ptr() if dev else None, k.ws.ptr(), k.st), what)
        k.done(what)
        fx.assert_untouched("x")
        fo.assert_untouched("other")
        _assert_loss(out, prev, O.f32(weight) * loss, weight, loss, what)
        for f, mode, ref, before, name in ((fgx, gx_mode, gx, gx0, "grad_x"), (fgo, go_mode, go, go0, "grad_other")):
            if mode is None:
                f.assert_untouched(what + f": a {name} nobody asked for")
            else:
                _assert_grad(f, ref * s + (before.double() if mode == "add" else 0.0), what + ": " + name)


# ---- the non-finite flag ----
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 1023, 2097152 + 3, 2097152 + 7])
def test_nonfinite_flag(n):
    """one bad value in turn at the first element, at the last element of the vector body, at every element of the scalar tail and at the
    last element.  2 097 152 + 3: every lane of the capped grid holds one quad, the tail has three elements; + 7: one lane takes a second quad"""
    A, L, st = O.abi()
    x = torch.rand(n, generator=_gen(n)) - 0.5
    fin = torch.tensor([O.FLT_MAX, -O.FLT_MAX, 2.0 ** -149, -0.0])
    x[:min(n, 4)] = fin[:min(n, 4)]
    x[-min(n, 4):] = fin[:min(n, 4)]
    fx = Fenced(x)
    body = 4 * (n // 4)
    places = sorted({0, n - 1, *range(body, n)} | ({body - 1} if body else set()))

    def flag(prev, accumulate):
        f = Fenced(torch.tensor([prev]))
        A.check(L.srganfd_nonfinite_flag(fx.ptr(), n, f.ptr(), accumulate, st), "nonfinite_flag")
        torch.cuda.synchronize()
        f.assert_fences("the floats around the flag")
        return f.val.item()

    assert O.nonfinite(x) == 0.0
    assert flag(SENTINEL, 0) == 0.0, "finite data (+-FLT_MAX, a denormal) flagged"
    assert flag(0.0, 1) == 0.0 and flag(1.0, 1) == 1.0, "accumulate keeps what the flag held"
    for at in places:
        for bad in (float("inf"), -float("inf"), float("nan")):
            keep = fx.val[at].item()
            fx.val[at] = bad
            assert O.nonfinite(fx.val) == 1.0
            assert flag(SENTINEL, 0) == 1.0, f"{bad} at {at} of {n} not seen"
            assert flag(0.0, 1) == 1.0, f"{bad} at {at} of {n} not seen when accumulating"
            fx.val[at] = keep
    assert flag(SENTINEL, 0) == 0.0
    fx.assert_fences("x")


# ---- the loss scaler ----
@pytest.mark.parametrize("seq", O.SCALE_SEQUENCES, ids=O.SCALE_IDS)
def test_loss_scale_update_word_for_word(seq):
    """the oracle's sequences (pinned to torch._amp_update_scale_ by tests/test_step_host.py) on the device state: all 8 words after every
    call, the counters as int32 words, the growth that would overflow included"""
    A, L, st = O.abi()
    start, founds, growth, backoff, interval = seq
    want = O.scale_state(start)
    dev = torch.full((16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    dev[4:12] = torch.from_numpy(want)
    found = torch.zeros(1, device="cuda")
    for i, f in enumerate(founds):
        found.fill_(float(f))
        A.check(L.srganfd_loss_scale_update(dev[4:12].data_ptr(), found.data_ptr(), growth, backoff, interval, st), "loss_scale_update")
        torch.cuda.synchronize()
        want = O.loss_scale_update(want, float(f), growth, backoff, interval)
        got = dev.cpu().numpy()
        assert (got[:4] == 0x5A5A5A5A).all() and (got[12:] == 0x5A5A5A5A).all(), "written outside the 8-word state"
        assert got[4:12].tolist() == want.tolist(), f"call {i} (found_inf = {f}): {got[4:12].tolist()} ({got[4:6].view(np.float32)}) against {want.tolist()} ({want[:2].view(np.float32)})"
        assert found.item() == float(f)
