"""tests/step_oracle.py against torch's own float64 operators on the CPU: the GPU tests of the elementwise, loss and optimizer kernels
trust these definitions.  Arithmetic is held to 1e-12 relative to the largest reference value, selections are exact."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import step_oracle as O

F64 = torch.float64


def _close(got, want, what, tol=1e-12):
    got, want = torch.as_tensor(got, dtype=F64), torch.as_tensor(want, dtype=F64)
    assert got.shape == want.shape, what
    e = ((got - want).abs().max() / (want.abs().max() + 1e-300)).item()
    assert e <= tol, f"{what}: {e:.3e}"


def _same(got, want, what):
    """exactly torch's values, NaN for NaN and the sign of a zero included"""
    got, want = torch.as_tensor(got, dtype=F64), torch.as_tensor(want, dtype=F64)
    assert torch.equal(torch.isnan(got), torch.isnan(want)), what + ": NaNs differ"
    assert torch.equal(torch.nan_to_num(got, nan=7.0), torch.nan_to_num(want, nan=7.0)), what
    ok = ~torch.isnan(want)
    assert torch.equal(torch.signbit(got[ok]), torch.signbit(want[ok])), what + ": signs of zero differ"


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64) * scale


SPECIAL = torch.tensor(O.SPECIAL, dtype=F64)


@pytest.mark.parametrize("dtype", O.DTYPES, ids=O.IDS)
@pytest.mark.parametrize("with_skip", [False, True])
def test_lrelu_backward_is_atens(dtype, with_skip):
    """ATen's leaky_relu_backward on z = act - skip (autograd through F.leaky_relu): the selection is exact, 0, -0 and NaN on the slope side"""
    z = _rand(5, 7, 16, seed=1).to(dtype)
    z.view(-1)[:len(SPECIAL)] = SPECIAL.to(dtype)
    skip = _rand(5, 7, 16, seed=2).to(dtype) if with_skip else None
    # act = z + skip would round: build act first and let z be whatever act - skip is
    act = z if skip is None else (z.double() + skip.double()).to(dtype)
    if with_skip:
        act.view(-1)[40:44] = skip.view(-1)[40:44]                                   # exact ties: act - skip = 0
    dy = _rand(5, 7, 16, seed=3).to(dtype)
    zz = (act.double() - (skip.double() if with_skip else 0.0)).requires_grad_(True)
    F.leaky_relu(zz, 0.2).backward(dy.double())
    got = O.lrelu_backward(dy, act, skip, 0.2)
    finite = torch.isfinite(zz.detach())
    _same(got[finite], zz.grad[finite], "lrelu_backward")
    # torch propagates nothing special for a NaN or infinite pre-activation either: `self > 0` decides
    want = torch.where(zz.detach() > 0, dy.double(), dy.double() * 0.2)
    _same(got, want, "lrelu_backward at NaN / inf")
    if with_skip:
        assert torch.equal(got.view(-1)[40:44], dy.double().view(-1)[40:44] * 0.2)


def test_axpby_sigmoid_and_its_backward():
    x, y = _rand(3, 50, seed=4), _rand(3, 50, seed=5)
    _close(O.axpby(x, y, 0.75, -1.5), 0.75 * x - 1.5 * y, "axpby")
    ynan = y.clone()
    ynan[0, :5] = float("nan")
    _same(O.axpby(x, ynan, 2.0, 0.0), 2.0 * x, "axpby with beta = 0 does not read y")
    _same(O.axpby(x.to(torch.float16), y.to(torch.bfloat16), 1.0, 1.0), x.to(torch.float16).double() + y.to(torch.bfloat16).double(), "axpby widens")
    pts = torch.tensor([0.0, -0.0, 1e-3, -1e-3, 20.0, -20.0, 90.0, -90.0, 104.0, -104.0, 800.0, -800.0, float("inf"), -float("inf")], dtype=F64)
    s = O.sigmoid(torch.cat([pts, x.view(-1) * 5]))
    _close(s, torch.sigmoid(torch.cat([pts, x.view(-1) * 5])), "sigmoid")
    assert torch.isfinite(s).all() and s[-1 - x.numel()] == 0 and s[-2 - x.numel()] == 1 and 0 < s[9] < 1e-44
    assert torch.isnan(O.sigmoid(torch.tensor([float("nan")]))).all()
    xr = (x * 4).requires_grad_(True)
    sr = torch.sigmoid(xr)
    sr.backward(y)
    _close(O.sigmoid_backward(y, sr.detach()), xr.grad, "sigmoid_backward")


@pytest.mark.parametrize("n", [1, 2, 65, 1000])
def test_l1_and_its_gradients(n):
    a, b = _rand(n, seed=6), _rand(n, seed=7)
    if n > 2:
        b[:2] = a[:2]                                                                # ties: gradient 0
    ar = a.clone().requires_grad_(True)
    ref = 20.0 * F.l1_loss(ar, b)
    ref.backward()
    loss, grad = O.l1(a, b, 20.0)
    _close(loss, ref.detach(), "l1")
    _close(grad, ar.grad, "l1 gradient")
    assert n <= 2 or (grad[:2] == 0).all()
    _close(O.l1_grad_views(a, b, 20.0 / n), ar.grad, "l1_grad_views")
    _close(O.l1_grad_views(a, b, 20.0 / n, upstream=torch.tensor(-3.0)), -3.0 * ar.grad, "l1_grad_views with an upstream gradient")
    _close(O.l1_views(a.view(n, 1), b.view(n, 1)), F.l1_loss(a, b), "l1_views")
    _close(O.l1_views(a, b, True), F.l1_loss(torch.relu(a), torch.relu(b)), "l1_views after relu")


def test_l1_follows_torch_at_special_values():
    a = SPECIAL.clone()
    b = torch.zeros_like(a)
    _same(O.sign(a), torch.sign(a), "sign")
    _same(O.relu(a), torch.relu(a), "relu")
    ar = a.clone().requires_grad_(True)
    F.l1_loss(ar, b).backward()
    loss, grad = O.l1(a, b)
    assert torch.isnan(loss) and torch.isnan(F.l1_loss(a, b))
    _same(grad, ar.grad, "l1 gradient at special values")
    assert grad[2] == 0 and grad[0] == 0 and grad[1] == 0                          # torch's sign is 0 at a NaN: the gradient does not carry it, the loss does
    assert torch.isnan(O.l1_views(a, b, True)) and torch.isnan(F.l1_loss(torch.relu(a), torch.relu(b)))
    fin = torch.tensor([1.0, -2.0, float("nan"), 3.0], dtype=F64)
    _same(O.l1_grad_views(fin, torch.ones(4, dtype=F64), 0.5), 0.5 * torch.sign(fin - 1), "l1_grad_views at a tie and a NaN")
    for bad in SPECIAL[~torch.tensor(O.SPECIAL_FINITE)]:
        assert O.nonfinite(torch.tensor([1.0, bad.item(), 2.0])) == 1.0
    assert O.nonfinite(SPECIAL[torch.tensor(O.SPECIAL_FINITE)].float()) == 0.0


@pytest.mark.parametrize("target", [0.0, 1.0])
@pytest.mark.parametrize("n", [1, 2, 16, 257])
def test_bce_and_its_gradients(n, target):
    x = _rand(n, seed=8, scale=3.0)
    if n >= 16:
        x[:4] = torch.tensor([90.0, -90.0, 0.0, 1e-3], dtype=F64)
    xr = x.clone().requires_grad_(True)
    ref = F.binary_cross_entropy_with_logits(xr, torch.full_like(x, target))
    ref.backward()
    loss, sig, grad = O.bce(x, target)
    _close(loss, ref.detach(), "bce")
    _close(grad, xr.grad, "bce gradient")
    _close(sig, torch.sigmoid(x).mean(), "mean sigmoid")
    _close(O.sigmoid_of_mean(x), torch.sigmoid(x.mean()), "sigmoid of the mean")


@pytest.mark.parametrize("target", [0.0, 1.0])
@pytest.mark.parametrize("n,n_other", [(1, 1), (16, 16), (16, 5), (7, 300)])
def test_relativistic_bce_and_both_gradients(n, n_other, target):
    x, other = _rand(n, seed=9, scale=3.0), _rand(n_other, seed=10, scale=3.0) + 0.5
    if n >= 16:
        x[:2] = torch.tensor([90.0, -90.0], dtype=F64)
    xr, otr = x.clone().requires_grad_(True), other.clone().requires_grad_(True)
    ref = F.binary_cross_entropy_with_logits(xr - otr.mean(), torch.full_like(x, target))
    ref.backward()
    loss, gx, go = O.bce_relativistic(x, other, target)
    _close(loss, ref.detach(), "relativistic bce")
    _close(gx, xr.grad, "relativistic bce, gradient of x")
    _close(go, otr.grad, "relativistic bce, gradient of other")


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.9)])
@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_adam_step_is_torch_optim_adam_and_the_ema_the_references_avg_fn(wd, betas):
    """five steps one at a time, each from torch's own state; the EMA through AveragedModel with the reference's avg_fn
    (train_bsrnet.py: (1 - decay) * averaged + decay * current; its first update is a copy)"""
    from torch.optim.swa_utils import AveragedModel
    d, lr, eps = 0.999, 0.05, 1e-3
    hp = dict(lr=lr, b1=betas[0], b2=betas[1], eps=eps, wd=wd, ema_decay=d)
    mod = torch.nn.Linear(40, 25, bias=False).double()
    with torch.no_grad():
        mod.weight.copy_(_rand(25, 40, seed=11, scale=0.1))
    opt = torch.optim.Adam(mod.parameters(), lr, betas, eps, wd)
    ema_model = AveragedModel(mod, avg_fn=lambda averaged, current, num: (1 - d) * averaged + d * current)
    p, m, v, ema = mod.weight.detach().clone(), torch.zeros(25, 40, dtype=F64), torch.zeros(25, 40, dtype=F64), None
    for t in range(1, 6):
        g = _rand(25, 40, seed=20 + t, scale=1e-2)
        mod.weight.grad = g.clone()
        opt.step()
        ema_model.update_parameters(mod)
        p, m, v, ema = O.adam_step(p, g * 4.0, m, v, ema, hp, t, grad_scale=0.25, ema_mode=1 if t == 1 else 2)
        state = opt.state[mod.weight]
        _close(p, mod.weight.detach(), f"p after step {t}")
        assert ((p - mod.weight.detach()).abs().max() <= 1e-12 * lr), f"the update of step {t}"
        _close(m, state["exp_avg"], f"m after step {t}")
        _close(v, state["exp_avg_sq"], f"v after step {t}")
        _close(ema, ema_model.module.weight.detach(), f"ema after step {t}")
        assert int(state["step"]) == t
    # a skipped step: p, m, v are the objects' own values, the EMA advances from the unchanged p
    p2, m2, v2, ema2 = O.adam_step(p, g, m, v, ema, hp, 6, ema_mode=2, skipped=True)
    assert torch.equal(p2, p) and torch.equal(m2, m) and torch.equal(v2, v)
    ema_model.update_parameters(mod)
    _close(ema2, ema_model.module.weight.detach(), "ema after a skipped step")
    assert O.adam_step(p, g, m, v, ema, hp, 6, ema_mode=0)[3] is ema
    b1f, b2f = O.f32(betas[0]), O.f32(betas[1])
    bc = O.bias_corrections(b1f, b2f, 3)
    assert bc[0].dtype == np.float32 and abs(float(bc[0]) - (1 - b1f ** 3)) < 1e-7 and abs(float(bc[1]) ** 2 - (1 - b2f ** 3)) < 1e-7


def _torch_scale_updates(scale, founds, growth, backoff, interval):
    s, tr = torch.tensor([scale], dtype=torch.float32), torch.zeros(1, dtype=torch.int32)
    out = []
    for f in founds:
        torch._amp_update_scale_(s, tr, torch.tensor([float(f)]), growth, backoff, interval)
        out.append((s.clone(), int(tr)))
    return out


@pytest.mark.parametrize("seq", O.SCALE_SEQUENCES, ids=O.SCALE_IDS)
def test_loss_scale_update_is_torchs_amp_update_scale(seq):
    start, founds, growth, backoff, interval = seq
    st = O.scale_state(start)
    assert st.dtype == np.int32 and st.shape == (8,) and st.view(np.float32)[1] == np.float32(1.0) / np.float32(start)
    want = _torch_scale_updates(start, founds, growth, backoff, interval)
    kept = False
    for k, f in enumerate(founds):
        prev = st.view(np.float32)[0]
        st = O.loss_scale_update(st, float(f), growth, backoff, interval)
        fl = st.view(np.float32)
        assert np.isfinite(fl[0]) and fl[0].tobytes() == want[k][0].numpy()[0].tobytes(), f"scale after call {k}"
        assert st[2] == want[k][1], f"growth tracker after call {k}"
        assert fl[1] == np.float32(1.0) / fl[0] and st[3] == k + 1 and st[4] == sum(founds[:k + 1]) and not st[5:].any()
        kept |= (not f) and st[2] == 0 and fl[0] == prev
    assert kept == (start * growth > O.FLT_MAX), "a growth past FLT_MAX keeps the scale and restarts the tracker, and only that does"
