"""csrc/norm.hip's BatchNorm entry points (plain, fused with LeakyReLU, two-phase) against the float64 definitions of
tests/norm_oracle.py: every dtype, one and two 16-byte chunks per pixel up to ragged channel blocks, every trip count of the
statistics loop, channel-slice views with sentinels around them, eval mode, gradient accumulation, unequal ranks, refusals that
must leave no trace, and the conditioning of the one-pass variance.

Bounds (norm_oracle.assert_f32 / assert_stored): fp32 results within 1e-5 (forward) or 1e-4 (backward) of float64 relative to
max|ref|; a stored 16-bit y or dx within one ulp of its type at |ref| on top of that."""
import pytest
import torch

from tests import norm_oracle as O

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]
WS_FLOATS = 2048 * 256 + 768             # 1024 blocks x 2 sums x 256 channels + the 3 x 256 backward coefficients
MOMENTUM, EPS, SLOPE = 0.1, 1e-5, 0.2
SENTINEL, Slot, _abi, _code = O.SENTINEL, O.Slot, O.abi, O.code


def make_case(dtype, c, npix, seed, device="cpu", zero_channel=None):
    """x and dy (npix, c) in ``dtype`` with a per-channel offset and scale, gamma and beta per channel: any mix-up of channels changes
    the result.  zero_channel: gamma = beta = 0 there.
    x is standardised over the pixels it has before the offset and scale go on, so every channel's mean/std is sin(ch) / (0.5 .. 1.5),
    at most 2, at every pixel count: three random pixels alone reach ratios of 20 to 90, where the one-pass variance is no longer good
    to 1e-5 (an fp32 emulation of its formula on the CPU shows the same loss).  That envelope is test_conditioning_of_the_one_pass_variance's
    subject; every other test here checks indexing, trip counts and views on well-conditioned data."""
    g = torch.Generator(device=device).manual_seed(seed)
    ch = torch.arange(c, dtype=torch.float32, device=device)
    z = torch.randn(npix, c, generator=g, device=device)
    if npix > 1:
        z = (z - z.mean(0)) / z.std(0, unbiased=False)
    x = (z * (0.5 + (ch % 7) / 6) + torch.sin(ch)).to(dtype)
    dy = (torch.randn(npix, c, generator=g, device=device) * (0.5 + (ch % 3) / 2)).to(dtype)
    gamma, beta = 0.5 + (ch % 5) / 4, torch.cos(ch * 0.7)
    if zero_channel is not None:
        gamma[zero_channel] = beta[zero_channel] = 0.0
    return x, dy, gamma, beta


def unblock(save, c):
    """the library's save, [block of 256][mean | invstd | scale | shift], as the oracle's [mean | invstd | scale | shift] over all c"""
    rows = [save[4 * cb:4 * cb + 4 * min(256, c - cb)].view(4, -1) for cb in range(0, c, 256)]
    return torch.cat(rows, dim=1).reshape(-1)


def assert_save(save, ref, c, what):
    got = unblock(save, c)
    for k, name in enumerate(("mean", "invstd", "scale", "shift")):
        O.assert_f32(got[k * c:(k + 1) * c], ref[k * c:(k + 1) * c], O.TOL_FWD, f"{what} save.{name}")


class Call:
    """buffers of one forward + backward through the library; plain entry points when slope is None, the fused ones otherwise"""

    def __init__(self, dtype, c, npix, x, dy, gamma, beta, slope=None, pad=0, c0s=(0, 0, 0, 0, 0), rm=None, rv=None):
        self.A, self.L, self.st = _abi()
        self.dtype, self.c, self.npix, self.slope = dtype, c, npix, slope
        self.x, self.y, self.dy, self.dx, self.act = (Slot((npix, c), dtype, d, pad, c0) for d, c0 in zip((x, None, dy, None, None), c0s))
        self.gamma, self.beta = gamma.float().cuda(), beta.float().cuda()
        self.rm = torch.zeros(c, device="cuda") if rm is None else rm.float().cuda()
        self.rv = torch.ones(c, device="cuda") if rv is None else rv.float().cuda()
        self.rm0, self.rv0 = self.rm.clone(), self.rv.clone()
        self.save = torch.full((4 * c,), SENTINEL, device="cuda")
        self.ws = torch.zeros(WS_FLOATS, device="cuda")
        self.dg, self.db = torch.full((c,), SENTINEL, device="cuda"), torch.full((c,), SENTINEL, device="cuda")

    def fwd(self, training=1):
        A, L = self.A, self.L
        args = (self.x.view(A), self.y.view(A), _code(A, self.dtype), self.npix, self.c, self.gamma.data_ptr(), self.beta.data_ptr(), self.rm.data_ptr(),
                self.rv.data_ptr(), MOMENTUM, EPS, training, self.save.data_ptr(), self.ws.data_ptr())
        if self.slope is None:
            A.check(L.srganfd_batchnorm_fwd(*args, self.st), "batchnorm_fwd")
        else:
            A.check(L.srganfd_batchnorm_act_fwd(*args, self.slope, self.st), "batchnorm_act_fwd")

    def bwd(self, acc=0.0):
        A, L = self.A, self.L
        args = (self.x.view(A), self.dy.view(A), self.dx.view(A), _code(A, self.dtype), self.npix, self.c, self.gamma.data_ptr(), self.save.data_ptr(),
                self.dg.data_ptr(), self.db.data_ptr(), acc, self.ws.data_ptr())
        if self.slope is None:
            A.check(L.srganfd_batchnorm_bwd(*args, self.st), "batchnorm_bwd")
        else:
            self.act.val.copy_(self.y.val)                       # the kernel's own forward output, also what the reference is given
            self.act.before.copy_(self.act.buf)
            A.check(L.srganfd_batchnorm_act_bwd(*args, self.act.view(A), self.slope, self.st), "batchnorm_act_bwd")

    def check_training(self, what, ref_device="cpu", old=None, acc=0.0):
        """everything a training-mode forward + backward wrote, against the float64 definitions"""
        torch.cuda.synchronize()
        dev, c = ref_device, self.c
        slope = 1.0 if self.slope is None else self.slope
        x, dy, gamma = self.x.val.to(dev), self.dy.val.to(dev), self.gamma.to(dev)
        y, rm, rv, save = O.bn_forward(x, gamma, self.beta.to(dev), self.rm0.to(dev), self.rv0.to(dev), MOMENTUM, EPS, True, slope)
        O.assert_stored(self.y.val, y, O.TOL_FWD, f"{what} y")
        O.assert_f32(self.rm, rm, O.TOL_FWD, f"{what} running_mean")
        O.assert_f32(self.rv, rv, O.TOL_FWD, f"{what} running_var")
        assert_save(self.save, save, c, what)
        dx, dgamma, dbeta = O.bn_backward(x, dy, gamma, save, act=None if self.slope is None else self.y.val.to(dev), slope=slope)
        if old is not None:
            dgamma, dbeta = dgamma + acc * old[0].double().to(dev), dbeta + acc * old[1].double().to(dev)
        O.assert_stored(self.dx.val, dx, O.TOL_BWD, f"{what} dx")
        O.assert_f32(self.dg, dgamma, O.TOL_BWD, f"{what} dgamma")
        O.assert_f32(self.db, dbeta, O.TOL_BWD, f"{what} dbeta")
        for s, name in ((self.x, "x"), (self.y, "y"), (self.dy, "dy"), (self.dx, "dx"), (self.act, "act")):
            s.assert_outside_untouched(f"{what} {name}")
        self.x.assert_untouched(f"{what} x")
        self.dy.assert_untouched(f"{what} dy")


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "lrelu"])
@pytest.mark.parametrize("c", [8, 64, 256, 264, 384, 512])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_every_dtype_and_channel_blocking(dtype, c, fused):
    """one or two 16-byte chunks per pixel, a full 256-channel block, ragged last blocks of 8 and 128, two full blocks; 210 pixels.
    The fused form has one channel with gamma = beta = 0: its output is exactly 0 and LeakyReLU'(0) is the slope, as in ATen."""
    npix, zc = 210, c // 2 + 1
    x, dy, gamma, beta = make_case(dtype, c, npix, seed=c, zero_channel=zc if fused else None)
    k = Call(dtype, c, npix, x, dy, gamma, beta, slope=SLOPE if fused else None)
    k.fwd()
    k.bwd()
    k.check_training(f"c={c}")
    if fused:
        assert (k.y.val[:, zc] == 0).all()
        dbeta_zc = SLOPE * dy[:, zc].double().sum().item()      # every element of that channel took the slope
        assert abs(k.db[zc].item() - dbeta_zc) <= O.TOL_BWD * k.db.abs().max().item()


def _pass_sizes(dtype):
    lanes = 4 if dtype == torch.float32 else 8               # pixels per block pass at c = 256
    step = 1024 * lanes                                      # pixels per grid pass of the statistics kernel
    return [3, step - 1, step + 1, 2 * step + 3, 3 * step + lanes + 1]


@pytest.mark.parametrize("which", range(5), ids=["under_one_row", "tail_only", "one_trip", "trip_and_tail", "second_trip"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_every_trip_count_of_the_statistics_loop(dtype, which):
    """c = 256: the forward statistics loop takes two grid passes per trip plus a one-pass tail; these pixel counts give fewer pixels
    than one block row, the tail alone, one trip without tail, one trip plus tail and a partial second trip"""
    c, npix = 256, _pass_sizes(dtype)[which]
    x, dy, gamma, beta = make_case(dtype, c, npix, seed=100 + which, device="cuda")
    k = Call(dtype, c, npix, x, dy, gamma, beta)
    k.fwd()
    k.bwd()
    k.check_training(f"npix={npix}", ref_device="cuda")


def test_grid_stride_apply_past_the_block_cap():
    """fp16, c = 8: 16384 * 256 + 777 pixels are more than the apply kernel's 16384 blocks of 256 pixels cover in one stride, and 17 grid
    passes of the statistics kernel"""
    dtype, c, npix = torch.float16, 8, 16384 * 256 + 777
    x, dy, gamma, beta = make_case(dtype, c, npix, seed=7, device="cuda")
    k = Call(dtype, c, npix, x, dy, gamma, beta)
    k.fwd()
    k.bwd()
    k.check_training("grid-stride", ref_device="cuda")


@pytest.mark.parametrize("c", [64, 384])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_channel_slice_views_are_honoured_and_nothing_else_is_written(dtype, c):
    """x, y, dy, dx and act each in a buffer of its own, c + 32 channels wide, at channel offsets 16, 8, 24, 0 and 16; c = 384 adds the
    second channel block's offset to a non-zero c0"""
    npix = 210
    x, dy, gamma, beta = make_case(dtype, c, npix, seed=31 + c, zero_channel=5)
    k = Call(dtype, c, npix, x, dy, gamma, beta, slope=SLOPE, pad=32, c0s=(16, 8, 24, 0, 16))
    k.fwd()
    k.bwd()
    k.check_training(f"views c={c}")
    assert (k.y.buf[:, :8] == SENTINEL).all() and (k.y.buf[:, 8 + c:] == SENTINEL).all() and (k.dx.buf[:, c:] == SENTINEL).all()


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "lrelu"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_eval_mode_uses_and_keeps_the_running_statistics(dtype, fused):
    c, npix = 264, 210
    x, dy, gamma, beta = make_case(dtype, c, npix, seed=5)
    g = torch.Generator().manual_seed(6)
    rm, rv = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    k = Call(dtype, c, npix, x, dy, gamma, beta, slope=SLOPE if fused else None, rm=rm, rv=rv)
    k.fwd(training=0)
    torch.cuda.synchronize()
    y, _, _, save = O.bn_forward(x, gamma, beta, rm, rv, MOMENTUM, EPS, False, SLOPE if fused else 1.0)
    O.assert_stored(k.y.val, y, O.TOL_FWD, "eval y")
    assert torch.equal(O.bits(k.rm), O.bits(k.rm0)) and torch.equal(O.bits(k.rv), O.bits(k.rv0))
    assert_save(k.save, save, c, "eval")
    assert torch.equal(unblock(k.save, c)[:c].cpu(), rm)                      # the mean slot is the running mean itself
    assert (unblock(k.save, c)[:c].cpu() - x.double().mean(0)).abs().max() > 0.1   # and not the batch's


@pytest.mark.parametrize("acc", [1.0, 0.5, 0.0])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_parameter_gradient_accumulation(dtype, acc):
    """dgamma/dbeta = sum + acc * old; acc = 0 stores plainly (old = NaN must not leak as 0 * NaN)"""
    c, npix = 264, 210
    x, dy, gamma, beta = make_case(dtype, c, npix, seed=8)
    k = Call(dtype, c, npix, x, dy, gamma, beta, slope=SLOPE)
    g = torch.Generator().manual_seed(9)
    old = (torch.randn(c, generator=g) * 10, torch.randn(c, generator=g) * 10)
    k.fwd()
    if acc == 0.0:
        k.dg.fill_(float("nan"))
        k.db.fill_(float("nan"))
    else:
        k.dg.copy_(old[0])
        k.db.copy_(old[1])
    k.bwd(acc=acc)
    k.check_training(f"acc={acc}", old=old, acc=acc)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_two_phase_form_with_unequal_ranks(dtype):
    """Two ranks holding 3 images and 1 image of 35 pixels, c = 256, fused slope; the all-reduce is emulated by adding the partial tables.
    Each rank passes its own npix and the shared total: outputs, running statistics and dx equal the full-batch float64 reference on both
    shares, and each rank's dgamma/dbeta are its own share's sums (the gradient all-reduce adds them later)."""
    A, L, st = _abi()
    c, hw, images = 256, 35, (3, 1)
    total = sum(images) * hw
    x, dy, gamma, beta = make_case(dtype, c, total, seed=77, zero_channel=9)
    x = (x.float() + torch.cat([torch.full((images[0] * hw, 1), 0.4), torch.full((images[1] * hw, 1), -1.2)])).to(dtype)   # the shares differ in mean
    nfl = L.srganfd_batchnorm_partial_floats(c)
    assert nfl == 2 * 1024 * c
    ranks, lo = [], 0
    for n in images:
        k = Call(dtype, c, n * hw, x[lo:lo + n * hw], dy[lo:lo + n * hw], gamma, beta, slope=SLOPE)
        k.wsg = torch.zeros(nfl, device="cuda")
        ranks.append(k)
        lo += n * hw

    def fwd(k, phase, tot):
        A.check(L.srganfd_batchnorm_fwd_sync(k.x.view(A), k.y.view(A), _code(A, dtype), k.npix, k.c, k.gamma.data_ptr(), k.beta.data_ptr(), k.rm.data_ptr(),
                                             k.rv.data_ptr(), MOMENTUM, EPS, k.save.data_ptr(), k.ws.data_ptr(), SLOPE, phase, tot, st), "fwd_sync")

    def bwd(k, phase, tot):
        A.check(L.srganfd_batchnorm_bwd_sync(k.x.view(A), k.dy.view(A), k.dx.view(A), _code(A, dtype), k.npix, k.c, k.gamma.data_ptr(), k.save.data_ptr(),
                                             k.dg.data_ptr(), k.db.data_ptr(), 0.0, k.ws.data_ptr(), k.wsg.data_ptr(), k.y.view(A), SLOPE, phase, tot, st), "bwd_sync")

    for k in ranks:
        fwd(k, 1, 0)
    table = ranks[0].ws[:nfl] + ranks[1].ws[:nfl]
    for k in ranks:
        k.y.assert_untouched("phase 1 y")
        k.ws[:nfl] = table
        fwd(k, 2, total)
    for k in ranks:
        bwd(k, 1, 0)
    table = ranks[0].ws[:nfl] + ranks[1].ws[:nfl]
    for k in ranks:
        k.wsg.copy_(table)
        bwd(k, 2, total)
    torch.cuda.synchronize()
    y, rm, rv, save = O.bn_forward(x, gamma, beta, torch.zeros(c), torch.ones(c), MOMENTUM, EPS, True, SLOPE)
    act = torch.cat([k.y.val for k in ranks]).cpu()
    O.assert_stored(act, y, O.TOL_FWD, "two-phase y")
    dx, dgamma, dbeta = O.bn_backward(x, dy, gamma, save, act=act, slope=SLOPE)
    O.assert_stored(torch.cat([k.dx.val for k in ranks]).cpu(), dx, O.TOL_BWD, "two-phase dx")
    O.assert_f32(ranks[0].dg + ranks[1].dg, dgamma, O.TOL_BWD, "two-phase dgamma, ranks added")
    O.assert_f32(ranks[0].db + ranks[1].db, dbeta, O.TOL_BWD, "two-phase dbeta, ranks added")
    lo = 0
    for r, k in enumerate(ranks):
        O.assert_f32(k.rm, rm, O.TOL_FWD, f"rank {r} running_mean")
        O.assert_f32(k.rv, rv, O.TOL_FWD, f"rank {r} running_var")
        assert_save(k.save, save, c, f"rank {r}")
        sl = slice(lo, lo + k.npix)
        dx_r, dg_r, db_r = O.bn_backward(x[sl], dy[sl], gamma, save, act=act[sl], slope=SLOPE, total=total, global_sums=(dbeta, dgamma))
        O.assert_stored(k.dx.val, dx_r, O.TOL_BWD, f"rank {r} dx")
        O.assert_f32(k.dg, dg_r, O.TOL_BWD, f"rank {r} dgamma")
        O.assert_f32(k.db, db_r, O.TOL_BWD, f"rank {r} dbeta")
        lo += k.npix
    own = x[:images[0] * hw].double().mean(0)
    assert (own - x.double().mean(0)).abs().max() > 0.1             # the shares' own statistics are not the batch's
    # more than one channel block has no two-phase form
    wide = Call(dtype, 264, 70, *make_case(dtype, 264, 70, seed=78), slope=SLOPE)
    wide.wsg = torch.zeros(nfl, device="cuda")
    for phase in (1, 2):
        with pytest.raises(A.SrganfdError):
            fwd(wide, phase, 140)
        with pytest.raises(A.SrganfdError):
            bwd(wide, phase, 140)
    torch.cuda.synchronize()
    wide.y.assert_untouched("refused y")
    wide.dx.assert_untouched("refused dx")


REFUSALS = [
    # id, dtype, c, npix, c0 of every view, training, forward only
    ("f16_c280_three_chunk_tail", torch.float16, 280, 210, 0, 1, False),
    ("bf16_c280_three_chunk_tail", torch.bfloat16, 280, 210, 0, 1, False),
    ("f32_c268_three_chunk_tail", torch.float32, 268, 210, 0, 1, False),
    ("bf16_c4_half_a_chunk", torch.bfloat16, 4, 210, 0, 1, False),
    ("f16_c0_misaligned", torch.float16, 64, 210, 4, 1, False),
    ("f32_c0_misaligned", torch.float32, 64, 210, 2, 1, False),
    ("f32_one_pixel_training", torch.float32, 64, 1, 0, 1, True),
    ("bf16_one_pixel_training", torch.bfloat16, 264, 1, 0, 1, True),
]


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "lrelu"])
@pytest.mark.parametrize("case", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_a_refused_call_has_no_effect(case, fused):
    """SrganfdError, and y, dx, save, the running statistics, dgamma and dbeta keep their pre-fill bit for bit.  (Before the checks moved
    in front of the first launch, c = 280 / 268 had written the first 256 channels of all of them; one pixel in training mode was
    accepted and put 0 * inf = NaN into running_var.)"""
    _, dtype, c, npix, c0, training, fwd_only = case
    A = _abi()[0]
    x, dy, gamma, beta = make_case(dtype, c, npix, seed=11)
    g = torch.Generator().manual_seed(12)
    k = Call(dtype, c, npix, x, dy, gamma, beta, slope=SLOPE if fused else None, pad=32, c0s=(c0,) * 5,
             rm=torch.randn(c, generator=g), rv=torch.rand(c, generator=g) + 0.5)
    with pytest.raises(A.SrganfdError):
        k.fwd(training=training)
    torch.cuda.synchronize()
    k.y.assert_untouched("y")
    assert torch.equal(O.bits(k.rm), O.bits(k.rm0)), f"running_mean written: {k.rm[:4].tolist()}"
    assert torch.equal(O.bits(k.rv), O.bits(k.rv0)), f"running_var written: {k.rv[:4].tolist()}"
    assert (k.save == SENTINEL).all(), f"save written: {k.save[:4].tolist()}"
    if fwd_only:
        return
    k.save.copy_(torch.cat([torch.zeros(c), torch.ones(3 * c)]))          # what a backward that did run would read
    k.y.val.copy_(x)                                                      # and its act
    save0 = k.save.clone()
    with pytest.raises(A.SrganfdError):
        k.bwd()
    torch.cuda.synchronize()
    for sl, name in ((k.dx, "dx"), (k.x, "x"), (k.dy, "dy")):
        sl.assert_untouched(name)
    assert torch.equal(k.save, save0)
    assert (k.dg == SENTINEL).all() and (k.db == SENTINEL).all(), f"dgamma/dbeta written: {k.dg[:4].tolist()} {k.db[:4].tolist()}"


def test_one_pixel_is_fine_in_eval_mode():
    dtype, c = torch.float32, 64
    x, dy, gamma, beta = make_case(dtype, c, 1, seed=13)
    k = Call(dtype, c, 1, x, dy, gamma, beta, rm=torch.full((c,), 0.25), rv=torch.full((c,), 1.5))
    k.fwd(training=0)
    torch.cuda.synchronize()
    y = O.bn_forward(x, gamma, beta, k.rm0.cpu(), k.rv0.cpu(), MOMENTUM, EPS, False)[0]
    O.assert_stored(k.y.val, y, O.TOL_FWD, "one pixel, eval")
    assert torch.isfinite(k.rv).all() and torch.equal(k.rv, k.rv0)


def test_conditioning_of_the_one_pass_variance():
    """var = E[x^2] - mean^2 from fp32 sums loses (mean/std)^2 * 2^-23 of relative accuracy.  fp32, 12293 pixels of unit std around
    per-channel means 0, 4, 16 and 64: the kernel's variance (1 / invstd^2 - eps) may be off float64's by at most 4 x what the same
    formula gives with torch's fp32 sums on the CPU (floor 2^-22) -- the factor covers the different summation order; the CPU emulation,
    not the kernel, sets the scale.  DESIGN.md ("BatchNorm statistics: numerical envelope") records the figures."""
    c, npix, means = 8, 12293, (0.0, 4.0, 16.0, 64.0)
    g = torch.Generator().manual_seed(21)
    m = torch.tensor(means * 2)
    x = torch.randn(npix, c, generator=g) + m
    k = Call(torch.float32, c, npix, x, torch.zeros(npix, c), torch.ones(c), torch.zeros(c))
    k.fwd()
    torch.cuda.synchronize()
    invstd = k.save[c:2 * c].double().cpu()
    var_k = 1.0 / invstd ** 2 - EPS
    mean32 = x.sum(0) / npix
    var_cpu = ((x * x).sum(0) / npix - mean32 * mean32).double()
    x64 = x.double()
    var_64 = ((x64 - x64.mean(0)) ** 2).mean(0)
    err_k, err_cpu = ((var_k - var_64).abs() / var_64).view(2, 4).amax(0), ((var_cpu - var_64).abs() / var_64).view(2, 4).amax(0)
    for i, mu in enumerate(means):
        print(f"mean/std {mu:4.0f}: kernel variance rel err {err_k[i]:.2e}, fp32 one-pass on the CPU {err_cpu[i]:.2e}")
    for i, mu in enumerate(means):
        bound = 4.0 * max(err_cpu[i].item(), 2.0 ** -22)
        assert err_k[i].item() <= bound, f"mean/std {mu}: {err_k[i]:.3e} > {bound:.3e}"
