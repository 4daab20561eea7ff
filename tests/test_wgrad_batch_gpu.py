"""The dense blocks' weight-gradient MFMA launches batched (srganfd_conv2d_wgrad_partial_batch; engine.batch_wgrads).

One launch over njobs blocks must leave in every job's workspace exactly the slabs that njobs single launches of the same plan leave:
the kernel only decodes (job, split, channel group) from the workgroup id instead of (split, channel group).  So the first test asks
for equal bits after the same reduction, over ragged tiles, every split count that takes another path (1, fewer than the tiles, the
tiles, more than the tiles: clamped) and batches up to the kernel's eight jobs.  The rest: each job against the fp64 autograd
reference with the bound of test_kernels_gpu.test_wgrad_dense_block_fused, reproducibility, that every slab the reduction reads
was written, the refusals, and the generator's backward with batching on against off."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.test_kernels_gpu import _assert_close, _rt

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
SIZES = [(1, 12, 36), (3, 8, 40)]           # (n, h, w): 12 x 36 is ragged in both directions (8 x 32 tiles), 4 tiles; 3 x 8 x 40: 6 tiles
LO = {5: 0, 4: 64, 3: 96, 2: 128, 1: 160}   # dy channels of conv k in the stacked gradient [dY5(64) | dY4 | dY3 | dY2 | dY1]
ALPHAS = (0.2, 0.04)                        # conv5's scale: a dense block, the last block of an RRDB
NPARAM = sum((64 if k == 5 else 32) * (64 + 32 * (k - 1)) * 9 + (64 if k == 5 else 32) for k in range(1, 6))


def _planar(t, dtype):
    """NCHW cpu tensor -> the engine's dense-block buffer on the GPU: per image, 32-channel groups as planes of (h, w, 32)"""
    n, c, h, w = t.shape
    return t.view(n, c // 32, 32, h, w).permute(0, 1, 3, 4, 2).contiguous().to(dtype).cuda()


def _convs(alpha):
    convs, off = [], 0
    for k in (1, 2, 3, 4, 5):
        cin, cout = 64 + 32 * (k - 1), (64 if k == 5 else 32)
        convs.append(dict(ci_lo=0, cin=cin, co_lo=LO[k], cout=cout, dw_off=off, db_off=off + cout * cin * 9, co_dst=cout, ci_dst=cin,
                          alpha=(alpha if k == 5 else 1.0)))
        off += cout * cin * 9 + cout
    assert off == NPARAM
    return convs


@functools.lru_cache(maxsize=None)
def _inputs(size, dtype):
    """eight jobs' distinct inputs for one size and dtype: (cat, dy) on the CPU, the planar GPU buffers, and the fp64 autograd
    gradients of the five convs (conv5 unscaled) as one flat vector laid out like _convs' offsets.  Computed once, never written."""
    n, h, w = size
    gen = torch.Generator().manual_seed(1000 * h + w)
    jobs = []
    for _ in range(8):
        cat, dy = torch.randn(n, 192, h, w, generator=gen), torch.randn(n, 192, h, w, generator=gen)
        ref = []
        for k in (1, 2, 3, 4, 5):
            cin, cout = 64 + 32 * (k - 1), (64 if k == 5 else 32)
            wt = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
            b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
            F.conv2d(_rt(cat[:, :cin], dtype), wt, b, padding=1).backward(_rt(dy[:, LO[k]:LO[k] + cout], dtype))
            ref += [wt.grad.reshape(-1), b.grad]
        jobs.append((_planar(cat, dtype), _planar(dy, dtype), torch.cat(ref)))
    return jobs


@functools.lru_cache(maxsize=None)
def _plans(size, dtype, splits):
    from sr_gan_fd_amd import ops
    n, h, w = size
    return tuple(ops.WgradPlan("cuda", ops.DT[dtype], n, h, w, 192, 192, _convs(a), splits=splits) for a in ALPHAS)


def _views(job):
    from sr_gan_fd_amd import _abi as A
    return A.View(job[0].data_ptr(), 192, 0, 1, 0), A.View(job[1].data_ptr(), 192, 0, 1, 0)


def _batched(plans, jobs, wss):
    """one batched launch over ``jobs`` (job j runs plans[j]), slabs into wss[j]"""
    from sr_gan_fd_amd import _abi as A
    arr = (A.WgradPartialJob * max(1, len(jobs)))()
    for j, (q, job, ws) in enumerate(zip(arr, jobs, wss)):
        q.plan_host, q.plan_dev = C.addressof(plans[j].host), plans[j].dev.data_ptr()
        q.x, q.dy = _views(job)
        q.workspace, q.workspace_bytes = ws.data_ptr(), ws.numel()
    return arr


def _reduce(plans, wss, grads):
    from sr_gan_fd_amd import _abi as A
    arr = (A.WgradReduceJob * len(wss))()
    for j, (q, ws) in enumerate(zip(arr, wss)):
        q.plan_host, q.plan_dev, q.grads, q.scalars, q.workspace = C.addressof(plans[j].host), plans[j].dev.data_ptr(), grads[j].data_ptr(), None, ws.data_ptr()
    A.check(A.lib().srganfd_wgrad_reduce_batch(arr, len(wss), A.stream_ptr()), "wgrad_reduce_batch")


def _run(size, dtype, njobs, splits, batched, fill=0.0):
    """gradients (njobs, NPARAM) of jobs 0..njobs-1: one batched launch or njobs single ones, then ONE reduction of all of them.
    Job j takes the RRDB's last-block plan where j % 3 == 2, as the engine's blocks do: a batch mixes the two alpha plans."""
    from sr_gan_fd_amd import _abi as A
    L, st = A.lib(), A.stream_ptr()
    two = _plans(size, dtype, splits)
    plans = [two[1 if j % 3 == 2 else 0] for j in range(njobs)]
    jobs = _inputs(size, dtype)[:njobs]
    wss = [torch.full((two[0].workspace_bytes // 4,), fill, device="cuda").view(torch.uint8) for _ in range(njobs)]
    grads = torch.full((njobs, NPARAM), 7.0, device="cuda")
    if batched:
        A.check(L.srganfd_conv2d_wgrad_partial_batch(_batched(plans, jobs, wss), njobs, st), "conv2d_wgrad_partial_batch")
    else:
        for p, job, ws in zip(plans, jobs, wss):
            x, dy = _views(job)
            A.check(L.srganfd_conv2d_wgrad_partial(p.host, p.dev.data_ptr(), x, dy, ws.data_ptr(), ws.numel(), st), "conv2d_wgrad_partial")
    _reduce(plans, wss, grads)
    torch.cuda.synchronize()
    return grads


def _splits(size, kind):
    n, h, w = size
    ntiles = n * -(-w // 32) * -(-h // 8)
    return {"1": 1, "3": 3, "ntiles": ntiles, "ntiles+1": ntiles + 1}[kind]


@pytest.mark.parametrize("kind", ["1", "3", "ntiles", "ntiles+1"])
@pytest.mark.parametrize("njobs", [1, 2, 4, 8])
@pytest.mark.parametrize("size", SIZES, ids=["1x12x36", "3x8x40"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_batched_launch_equals_single_launches_bit_for_bit(dtype, size, njobs, kind):
    splits = _splits(size, kind)
    plan = _plans(size, dtype, splits)[0]
    assert plan.splits == min(splits, plan.ntiles)                  # more splits than tiles: clamped
    got, want = _run(size, dtype, njobs, splits, True), _run(size, dtype, njobs, splits, False)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)


@pytest.mark.parametrize("njobs", [4, 8])
@pytest.mark.parametrize("size", SIZES, ids=["1x12x36", "3x8x40"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_each_job_matches_fp64_autograd_and_runs_reproducibly(dtype, size, njobs):
    """against the fp64 reference with test_wgrad_dense_block_fused's bound; workspaces pre-filled with NaN: a slab the reduction
    reads and the launch did not write would show; two runs: equal bits"""
    got = _run(size, dtype, njobs, 3, True, fill=float("nan"))
    assert torch.isfinite(got).all()
    assert torch.equal(got, _run(size, dtype, njobs, 3, True, fill=float("nan")))
    off5 = _convs(1.0)[4]["dw_off"]
    for j, (_, _, ref) in enumerate(_inputs(size, dtype)[:njobs]):
        alpha = ALPHAS[1 if j % 3 == 2 else 0]
        for c in _convs(alpha):
            a = c["alpha"]
            lo, mid, hi = c["dw_off"], c["db_off"], c["db_off"] + c["cout"]
            _assert_close(got[j, lo:mid], a * ref[lo:mid], dtype, f"job {j} dW at {lo}")
            _assert_close(got[j, mid:hi], a * ref[mid:hi], dtype, f"job {j} db at {mid}")
        assert off5 == c["dw_off"]


def test_refusals():
    from sr_gan_fd_amd import _abi as A, ops
    L, st = A.lib(), A.stream_ptr()
    size, dtype = SIZES[0], torch.float16
    plans = [_plans(size, dtype, 3)[0]] * 9
    jobs = (_inputs(size, dtype) + _inputs(size, dtype))[:9]
    wss = [torch.empty(plans[0].workspace_bytes, dtype=torch.uint8, device="cuda") for _ in range(2)] * 5
    call = lambda arr, n: A.check(L.srganfd_conv2d_wgrad_partial_batch(arr, n, st), "conv2d_wgrad_partial_batch")
    with pytest.raises(A.SrganfdError, match="jobs"):
        call(_batched(plans, jobs, wss), 0)
    with pytest.raises(A.SrganfdError, match="jobs"):
        call(_batched(plans, jobs, wss), 9)
    other = ops.WgradPlan("cuda", ops.DT[dtype], 1, 16, 36, 192, 192, _convs(0.2), splits=3)     # another height
    with pytest.raises(A.SrganfdError, match="geometry"):
        call(_batched([plans[0], other], jobs[:2], wss[:2]), 2)
    arr = _batched(plans[:2], jobs[:2], wss[:2])
    arr[1].workspace_bytes = plans[0].workspace_bytes - 4
    with pytest.raises(A.SrganfdError, match="workspace"):
        call(arr, 2)
    torch.cuda.synchronize()


# ---- end to end: the generator's backward with the batched launches against the per-block ones ----
def _flat_grad(monkeypatch, dt, batch, chain, prepare, x, dout):
    from sr_gan_fd_amd import engine as E, model as M, ops
    monkeypatch.setattr(E, "_BATCH_WGRAD", batch)
    monkeypatch.setattr(ops, "DENSE_CHAIN", chain)
    torch.manual_seed(0)
    g = M.bsrgan_x4(num_rrdb=2)
    prepare(g)
    g.compute_dtype = dt
    g.cuda()
    eng = E.generator_engine(g)
    eng.forward(x.cuda(), True)
    sp = eng._last
    kinds = [it.kind for it in sp.bw]
    assert ("wgrad_partial_batch" in kinds) == (batch == "1") and ("wgrad_partial" in kinds) == (batch == "0")
    grad, _ = eng.backward(sp, eng.token, dout.cuda(), True, False)
    torch.cuda.synchronize()
    assert torch.isfinite(grad).all()
    return grad.clone(), ("chain" in kinds), (eng.fp.off("trunk.0.rdb1.conv5.weight"), eng.fp.off("trunk.0.rdb1.conv5.bias"))


@pytest.mark.parametrize("chain", ["0", "1"], ids=["per-layer", "dense-chain"])
@pytest.mark.parametrize("dt", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_generator_backward_random_inputs(monkeypatch, dt, chain):
    """6 blocks at 2x3x16x16: batches of three blocks with one pixel split each against three launches with four.  The two differ by
    the grouping of fp32 sums only: every element is a sum of at most 2 * 16 * 16 = 2^9 products per tap, so reassociation moves it
    by at most ~2^9 * 2^-24 = 3e-5 of the sum of magnitudes in the worst case and by ~sqrt(2^9) * 2^-24 = 1.3e-6 for rounding errors
    of random sign; relative L2 over the whole gradient <= 1e-5"""
    torch.manual_seed(5)
    x, dout = torch.rand(2, 3, 16, 16), torch.randn(2, 3, 64, 64)
    on, chained, _ = _flat_grad(monkeypatch, dt, "1", chain, lambda g: None, x, dout)
    off, _, _ = _flat_grad(monkeypatch, dt, "0", chain, lambda g: None, x, dout)
    assert chained == (chain == "1" and dt != torch.float32)
    rel = ((on.double() - off.double()).norm() / off.double().norm()).item()
    print(f"batched vs per-block flat gradient, {dt}, dense chain {chain}: relative L2 {rel:.3e}")
    assert rel <= 1e-5


def _integer_net(g):
    """weights that keep every activation and gradient a small integer, so that the fp32 partial sums of the weight gradients are
    exact whatever their grouping: conv1 copies the image's channels, the growth convs copy a channel of the block input and add 1,
    conv5 is zero (a block passes its input on; an RRDB gives 1.2 x its input: inputs are multiples of 25), conv2 and the tail copy
    channels and conv4 scales by 2^-10 around 0.25, inside the clamp"""
    with torch.no_grad():
        for p in g.parameters():
            p.zero_()
        for c in range(64):
            g.conv1.weight[c, c % 3, 1, 1] = 1.0
        for m in g.modules():
            if hasattr(m, "conv5") and hasattr(m, "conv1") and m.conv1.weight.shape[0] == 32:
                for k in range(1, 5):
                    cv = getattr(m, "conv%d" % k)
                    for o in range(32):
                        cv.weight[o, o, 1, 1] = 1.0
                    cv.bias.fill_(1.0)
        for cv in (g.conv2, g.upsampling1[0], g.upsampling2[0], g.conv3[0]):
            for c in range(64):
                cv.weight[c, c, 1, 1] = 1.0
        for o in range(3):
            for c in range(o, 15, 3):                    # five channels each: 5 * 122 * 2^-10 + 0.25 < 1
                g.conv4.weight[o, c, 1, 1] = 2.0 ** -10
        g.conv4.bias.fill_(0.25)


@pytest.mark.parametrize("chain", ["0", "1"], ids=["per-layer", "dense-chain"])
@pytest.mark.parametrize("dt", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_generator_backward_exact_sums_give_equal_bits(monkeypatch, dt, chain):
    """small-integer activations and gradients (_integer_net; the image gradient is non-zero at one pixel of every 8 x 8, so the
    nearest adjoints sum one term): every dense block's weight gradient is a sum of at most 128 integer products below 2^12 --
    exact in fp32 in any order.  What the blocks compute: conv5's gradient (dOut x the block's 192 input channels, all nine taps);
    conv5 being zero, the growth convs' output gradients are zero."""
    torch.manual_seed(6)
    x = 25.0 * torch.randint(1, 3, (2, 3, 16, 16)).float()
    dout = torch.zeros(2, 3, 64, 64)
    dout[:, :, ::8, ::8] = 25.0 * 1024.0 * torch.randint(1, 3, (2, 3, 8, 8)).float()
    on, _, (lo, hi) = _flat_grad(monkeypatch, dt, "1", chain, _integer_net, x, dout)
    off, _, _ = _flat_grad(monkeypatch, dt, "0", chain, _integer_net, x, dout)
    assert float(on[lo:hi].abs().max()) > 0                                  # the blocks' gradients are not all zero
    assert torch.equal(on, off)
