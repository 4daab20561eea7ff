"""csrc/optim.hip's fused Adam + EMA step, both entry points, one step at a time against tests/step_oracle.adam_step (pinned to
torch.optim.Adam and AveragedModel by tests/test_step_host.py): the reference starts from the state the kernel started from, so nothing
compounds and the bounds stay tight.

Hyper-parameters that make every term matter: lr = 0.05 on p ~ 0.1 N(0, 1) with g ~ 1e-2 N(0, 1) and eps = 1e-3 (of the size of
sqrt(v)), weight decay 0 and 0.1, two pairs of betas, steps 1, 2 and 1000, grad_scale = 0.5 together with a device-resident 1 / 1024 on
a gradient multiplied by 2048, every EMA mode, the skip flag absent, 0 and 1.

Bounds (none measured on the code under test):
  m, v, ema     norm_oracle.assert_f32 at TOL_FWD
  p             |p - ref| <= ulp32(ref) + 1e-5 * max|ref - p0|: one rounding of the stored parameter plus the forward bound on the UPDATE,
                never relative to |p|
  a skipped step leaves the bits of p, m, v alone, advances the EMA from the unchanged p and (srganfd_adam_ema_dev) does not count

Which test reaches which launch (SRGANFD_LAUNCH lines of csrc/optim.hip):
  adam_ema_kernel                          test_adam_step_hyper_parameters, test_adam_step_sizes, test_adam_second_trip_of_the_grid
  adam_step_kernel, adam_ema_dev_kernel    the same three, and test_adam_dev_counts_steps_and_writes_the_bias_corrections"""
import numpy as np
import pytest
import torch

from tests import step_oracle as O

pytestmark = pytest.mark.gpu

Fenced, SENTINEL = O.Fenced, O.SENTINEL
GRID = 8192 * 256                                            # threads of the largest grid: one element more takes a second trip
LR, EPS, DECAY = 0.05, 1e-3, 0.999
UNSCALE = 1.0 / 1024.0


def _state(n, t, seed, device="cpu"):
    """(p, g, m, v, ema) before step t: the moments of a run that has seen gradients of this size (zero before the first step)"""
    gen = torch.Generator(device=device).manual_seed(seed)
    r = lambda: torch.randn(n, generator=gen, device=device)
    p, g = 0.1 * r(), 1e-2 * r()
    m, v = (torch.zeros(n, device=device), torch.zeros(n, device=device)) if t == 1 else (5e-3 * r(), 1e-4 * r() ** 2 + 1e-9)
    return p, g, m, v, p + 1e-2 * r()


def _bits_equal(a, b):
    return torch.equal(O.bits(a), O.bits(b))


def _step(entry, state, hp, t, ema_mode, skip, scaled):
    """one call of `entry` ("host": srganfd_adam_ema, "dev": srganfd_adam_ema_dev with the counter preset to t - 1), checked against the
    oracle.  skip: None (no flag), 0.0 or 1.0.  Returns the buffers (p, m, v, ema) and, for "dev", the two bias corrections."""
    A, L, st = O.abi()
    p0, g, m0, v0, e0 = state
    n = p0.numel()
    fp, fm, fv, fe = Fenced(p0), Fenced(m0), Fenced(v0), Fenced(e0)
    fg = Fenced(g * 2048.0 if scaled else g)                  # a power of two: the kernel's g * 0.5 * (1 / 1024) is g again, exactly
    gs, gsd = (0.5, torch.tensor([UNSCALE], device="cuda")) if scaled else (1.0, None)
    flag = torch.tensor([skip], device="cuda") if skip is not None else None
    common = (fp.ptr(), fg.ptr(), fm.ptr(), fv.ptr(), fe.ptr(), n, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"])
    tail = (gs, hp["ema_decay"], ema_mode, flag.data_ptr() if flag is not None else None, gsd.data_ptr() if gsd is not None else None, st)
    what = f"adam({entry}) n={n} t={t} wd={hp['wd']:.1f} b1={hp['b1']:.1f} ema_mode={ema_mode} skip={skip} scaled={scaled}"
    bc = None
    if entry == "host":
        A.check(L.srganfd_adam_ema(*common, t, *tail), what)
    else:
        step = torch.tensor([7, t - 1, 7], dtype=torch.int32, device="cuda")
        bc = Fenced(n=2)
        A.check(L.srganfd_adam_ema_dev(*common, step.data_ptr() + 4, bc.ptr(), *tail), what)
    torch.cuda.synchronize()
    skipped = bool(skip)
    if entry == "dev":
        assert step.tolist() == [7, t - 1 if skipped else t, 7], what + ": the step counter"
        bc.assert_fences(what + ": bc_dev")
        if skipped:
            bc.assert_untouched(what + ": bc_dev on a skipped step")
    fg.assert_untouched(what + ": the gradient")
    for f, name in ((fp, "p"), (fm, "m"), (fv, "v"), (fe, "ema")):
        f.assert_fences(what + ": " + name)
    p, m, v, ema = O.adam_step(p0, g, m0, v0, e0, hp, t, 1.0, ema_mode, skipped)
    if skipped:
        for f, name in ((fp, "p"), (fm, "m"), (fv, "v")):
            f.assert_untouched(what + f": {name} on a skipped step")
    else:
        got = fp.val.double().to(p.device)
        assert torch.isfinite(got).all(), what
        excess = ((got - p).abs() - O.ulp32(p) - 1e-5 * (p - p0.double()).abs().max()).max().item()
        print(f"{what}: p exceeds ulp32 + 1e-5 max|update| by {excess:.2e} (max|update| {(p - p0.double()).abs().max().item():.2e})")
        assert excess <= 0.0, what + ": p"
        O.assert_f32(fm.val, m, O.TOL_FWD, what + ": m")
        O.assert_f32(fv.val, v, O.TOL_FWD, what + ": v")
    if ema_mode == 0:
        fe.assert_untouched(what + ": the EMA with ema_mode = 0")
    else:
        O.assert_f32(fe.val, ema, O.TOL_FWD, what + ": ema")
        if ema_mode == 1:
            assert _bits_equal(fe.val, fp.val), what + ": ema_mode = 1 is a copy"
    return (fp.val, fm.val, fv.val, fe.val), (bc.val.cpu().numpy() if bc is not None and not skipped else None)


def _both_entries(state, hp, t, ema_mode, skip, scaled):
    host, _ = _step("host", state, hp, t, ema_mode, skip, scaled)
    dev, bc = _step("dev", state, hp, t, ema_mode, skip, scaled)
    if bc is None:                                            # skipped: nothing depends on the bias corrections
        same = True
    else:
        want = np.array(O.bias_corrections(hp["b1"], hp["b2"], t))
        same = bc.tobytes() == want.tobytes()
        print(f"bc_dev {bc.tolist()} against the host's {want.tolist()}: {'bit-equal' if same else 'DIFFERENT'}")
        assert (np.abs(bc.astype(np.float64) - want.astype(np.float64)) <= np.spacing(want)).all(), "bc_dev more than one fp32 step from the host's"
    if same:
        for a, b, name in zip(host, dev, ("p", "m", "v", "ema")):
            assert _bits_equal(a, b), f"srganfd_adam_ema and srganfd_adam_ema_dev differ in {name} (t={t}, ema_mode={ema_mode}, skip={skip})"
    return same


MODES = [(ema_mode, skip) for ema_mode in (0, 1, 2) for skip in (None, 0.0, 1.0)]


@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.9)], ids=["b.9-.999", "b.5-.9"])
def test_adam_step_hyper_parameters(betas, wd, t):
    hp = O.hyper(LR, betas[0], betas[1], EPS, wd, DECAY)
    state = _state(1000, t, seed=t)
    for ema_mode, skip in MODES:
        for scaled in (False, True):
            _both_entries(state, hp, t, ema_mode, skip, scaled)


@pytest.mark.parametrize("n", [1, 255, 257])
def test_adam_step_sizes(n):
    """one element, a block that is not full, one element into the second block (1000 is test_adam_step_hyper_parameters' size)"""
    hp = O.hyper(LR, 0.9, 0.999, EPS, 0.1, DECAY)
    for t in (1, 2):
        state = _state(n, t, seed=10 + n)
        for ema_mode, skip in MODES:
            _both_entries(state, hp, t, ema_mode, skip, scaled=bool(ema_mode % 2))


@pytest.mark.parametrize("skip", [None, 1.0], ids=["step", "skipped"])
def test_adam_second_trip_of_the_grid(skip):
    """2 097 152 + 37 elements on a grid capped at 8192 blocks of 256: the last 37 are the second trip's.  Reference on the device."""
    hp = O.hyper(LR, 0.9, 0.999, EPS, 0.1, DECAY)
    state = _state(GRID + 37, 2, seed=20, device="cuda")
    _both_entries(state, hp, 2, 2, skip, scaled=True)


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.9)], ids=["b.9-.999", "b.5-.9"])
def test_adam_dev_counts_steps_and_writes_the_bias_corrections(betas):
    """t calls from a counter at 0 (t = 1, 2, 3) and one from a counter preset to 999: *step_dev and bc_dev against the host's formula
    (float)(1 - b1^t), (float)sqrt(1 - b2^t) in double; a skipped call in between moves neither"""
    A, L, st = O.abi()
    hp = O.hyper(LR, betas[0], betas[1], EPS, 0.0, DECAY)
    n = 257
    p, g, m, v, _ = [x.cuda() for x in _state(n, 1, seed=30)]
    step, bc = torch.zeros(1, dtype=torch.int32, device="cuda"), Fenced(n=2)
    skip = torch.zeros(1, device="cuda")
    call = lambda: A.check(L.srganfd_adam_ema_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), None, n, hp["lr"], hp["b1"], hp["b2"], hp["eps"],
                                                  hp["wd"], step.data_ptr(), bc.ptr(), 1.0, hp["ema_decay"], 0, skip.data_ptr(), None, st), "adam_ema_dev")
    different = []
    for t in (1, 2, 3, 1000):
        if t == 1000:
            step.fill_(999)
        call()
        torch.cuda.synchronize()
        bc.assert_fences("bc_dev")
        got, want = bc.val.cpu().numpy(), np.array(O.bias_corrections(hp["b1"], hp["b2"], t))
        assert step.item() == t
        assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(want)).all(), f"t={t}: bc_dev {got.tolist()} against {want.tolist()}"
        if got.tobytes() != want.tobytes():
            different.append((t, got.tolist(), want.tolist()))
        if t == 2:                                            # a skipped call: the counter, the corrections and the parameters stay
            before = (p.clone(), bc.val.clone())
            skip.fill_(1.0)
            call()
            torch.cuda.synchronize()
            skip.fill_(0.0)
            assert step.item() == 2 and _bits_equal(bc.val, before[1]) and _bits_equal(p, before[0])
    print(f"bc_dev against the host's two floats, betas {betas}: " + ("bit-equal at t = 1, 2, 3, 1000" if not different else f"DIFFERENT at {different}"))
    assert torch.isfinite(p).all()
