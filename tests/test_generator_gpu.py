"""GPU parity of the generator path (dense blocks, RRDBNet / BSRGAN forward + backward through the
C ABI) against the golden vectors captured from the reference (tests/golden/*.npz).

Tolerances (relative to the tensor's max magnitude):
  f32 mode  (exact-fp32 MFMA): SR pixels / losses 1e-3 as BASELINE.json's north_star states (observed ~1e-5);
  f16 mode  (the benchmark dtype; the reference's autocast dtype): the same 1e-3;
  bf16 mode: reported and bounded at 1.5e-2 -- 8-bit mantissa through >=30 chained convs.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.util import checksum, load_golden, scaled_init, table

pytestmark = pytest.mark.gpu

# SR / loss bounds.  f32 and f16 carry BASELINE.json's tolerance (1e-3); bf16 cannot (8-bit mantissa through 351 chained convs:
# observed 5-7e-3 of the SR range) and is bounded at twice what is observed.  Gradients: f16 backward runs loss-scaled.
TOL = {torch.float32: 1e-3, torch.bfloat16: 1.5e-2, torch.float16: 1e-3}
# (the L1 loss gradient is sign(sr - gt) / n: a pixel whose |sr - gt| is below the forward error flips its +-1/n seed, and the bias
# gradients are sums of those signs with heavy cancellation -- this bound measures sign flips, not kernel rounding; the f32 row does)
GTOL = {torch.float32: 2e-3, torch.bfloat16: 2e-1, torch.float16: 1e-1}
LOSS_SCALE = {torch.float32: 1.0, torch.bfloat16: 1.0, torch.float16: 65536.0}   # what GradScaler does for the reference's fp16 autocast


def _rel(a, b):
    a = torch.as_tensor(np.asarray(a)).double().cpu() if not torch.is_tensor(a) else a.detach().double().cpu()
    b = torch.as_tensor(np.asarray(b)).double().cpu() if not torch.is_tensor(b) else b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("kind", ["rdb", "rrdb"])
def test_blocks(golden_dir, dtype, kind):
    from sr_gan_fd_amd import model as M
    g = load_golden(golden_dir, "blocks.npz")
    torch.manual_seed(0)
    blk = (M._ResidualDenseBlock if kind == "rdb" else M._ResidualResidualDenseBlock)(64, 32)
    blk.compute_dtype = dtype
    blk.cuda()
    x = torch.tensor(g[f"{kind}_x"]).cuda().requires_grad_(True)
    y = blk(x)
    e = _rel(y, g[f"{kind}_y"])
    print(f"{kind} {dtype}: y err {e:.2e}")
    assert e < TOL[dtype]
    (y * torch.tensor(g[f"{kind}_r"]).cuda()).sum().backward()
    e = _rel(x.grad, g[f"{kind}_dx"])
    print(f"{kind} {dtype}: dx err {e:.2e}")
    assert e < GTOL[dtype]
    named = dict(blk.named_parameters())
    first = "conv1" if kind == "rdb" else "rdb1.conv1"
    last = "conv5" if kind == "rdb" else "rdb3.conv5"
    assert _rel(named[first + ".weight"].grad, g[f"{kind}_g_first_w"]) < GTOL[dtype]
    assert _rel(named[last + ".bias"].grad, g[f"{kind}_g_last_b"]) < GTOL[dtype]
    if dtype == torch.float32:
        for k, want in table(g, f"{kind}_gsum").items():
            got = checksum(named[k].grad)
            assert np.allclose(got, want, rtol=5e-3, atol=2e-4 * abs(want[1])), f"{kind} grad checksum {k}: {got} vs {want}"


CASES = [
    ("bsrgan_x4_r2_s3", "bsrgan_x4", dict(num_rrdb=2), 4, 3.0),
    ("bsrgan_x2_r2_s3", "bsrgan_x2", dict(num_rrdb=2), 2, 3.0),
    ("bsrgan_x4_r2_s5", "bsrgan_x4", dict(num_rrdb=2), 4, 5.0),
    ("rrdbnet_x4_r23_s3", "rrdbnet_x4", dict(num_blocks=23), 4, 3.0),
    ("bsrgan_x4_r23_s3_odd", "bsrgan_x4", dict(num_rrdb=23), 4, 3.0),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name,fac,kw,s,scale", CASES)
def test_generator(golden_dir, dtype, name, fac, kw, s, scale):
    from sr_gan_fd_amd import model as M
    g = load_golden(golden_dir, "generator.npz")
    torch.manual_seed(0)
    net = getattr(M, fac)(in_channels=3, out_channels=3, channels=64, growth_channels=32, **kw)
    scaled_init(net, scale, 0.5)
    net.compute_dtype = dtype
    net.cuda()
    x, gt = torch.tensor(g[f"{name}/x"]).cuda(), torch.tensor(g[f"{name}/gt"]).cuda()
    sr = net(x)
    e = _rel(sr, g[f"{name}/sr"])
    psnr = 10 * np.log10(1.0 / max(((sr.detach().cpu().double() - torch.tensor(g[f"{name}/sr"]).double()) ** 2).mean().item(), 1e-20))
    print(f"{name} {dtype}: SR max err {e:.2e}, PSNR vs reference {psnr:.1f} dB")
    assert e < TOL[dtype]
    loss = torch.nn.functional.l1_loss(sr, gt)
    assert abs(loss.item() - float(g[f"{name}/loss"])) < TOL[dtype] * abs(float(g[f"{name}/loss"]))
    S = LOSS_SCALE[dtype]
    (loss * S).backward()
    named = dict(net.named_parameters())
    worst = 0.0
    for k in ("conv1.weight", "conv4.weight", "conv4.bias", "trunk.0.rdb1.conv1.bias", "trunk.1.rdb3.conv5.bias", "conv2.bias"):
        worst = max(worst, _rel(named[k].grad / S, g[f"{name}/grad/{k}"]))
    print(f"{name} {dtype}: worst grad err {worst:.2e}")
    assert worst < GTOL[dtype]
    if dtype == torch.float32:
        for k, want in table(g, f"{name}/gsum").items():
            got = checksum(named[k].grad)
            assert np.allclose(got, want, rtol=2e-2, atol=2e-3 * abs(want[1]) + 1e-12), f"{name} grad checksum {k}: {got} vs {want}"
    # inference path (rotating buffers) must give the same pixels as the training-mode forward
    with torch.no_grad():
        sr2 = net(x)
    assert torch.equal(sr2, sr.detach())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name,s", [("x2_r2_s3", 2), ("x1_r2_s3", 1), ("x2_r2_s3_odd", 2)])
def test_realesrgan_rrdbnet_below_x4(golden_dir, dtype, name, s):
    """Real-ESRGAN's RRDBNet at x2 / x1 (Real_ESRGAN/model.py:190-204,248-262: PixelUnshuffle(2 / 4) in front of conv1, which then reads
    12 / 48 channels; both upsampling stages) against outputs and gradients of the reference class; bounds TOL / GTOL as test_generator"""
    from sr_gan_fd_amd import model as M
    g = load_golden(golden_dir, "realesrgan_rrdbnet.npz")
    torch.manual_seed(0)
    net = M.RRDBNet(in_channels=3, out_channels=3, channels=64, growth_channels=32, num_rrdb=2, upscale_factor=s)
    scaled_init(net, 3.0, 0.5)
    net.compute_dtype = dtype
    net.cuda()
    x, gt = torch.tensor(g[f"{name}/x"]).cuda(), torch.tensor(g[f"{name}/gt"]).cuda()
    sr = net(x)
    assert sr.shape == gt.shape
    e = _rel(sr, g[f"{name}/sr"])
    print(f"Real-ESRGAN RRDBNet {name} {dtype}: SR max err {e:.2e}")
    assert e < TOL[dtype]
    loss = torch.nn.functional.l1_loss(sr, gt)
    assert abs(loss.item() - float(g[f"{name}/loss"])) < TOL[dtype] * abs(float(g[f"{name}/loss"]))
    S = LOSS_SCALE[dtype]
    (loss * S).backward()
    named = dict(net.named_parameters())
    worst = 0.0
    for k in ("conv1.weight", "conv1.bias", "conv4.weight", "trunk.0.rdb1.conv1.bias", "trunk.1.rdb3.conv5.bias", "conv2.bias"):
        worst = max(worst, _rel(named[k].grad / S, g[f"{name}/grad/{k}"]))
    print(f"Real-ESRGAN RRDBNet {name} {dtype}: worst grad err {worst:.2e}")
    assert worst < GTOL[dtype]


def test_state_dict_roundtrip_and_deepcopy(golden_dir):
    """the boundary: state_dict keys/shapes of the reference, deepcopy (AveragedModel), load_state_dict"""
    import copy
    from sr_gan_fd_amd import model as M
    g = load_golden(golden_dir, "generator.npz")
    torch.manual_seed(0)
    net = M.bsrgan_x4(num_rrdb=2)
    scaled_init(net, 3.0, 0.5)
    net.compute_dtype = torch.float32
    net.cuda()
    x = torch.tensor(g["bsrgan_x4_r2_s3/x"]).cuda()
    with torch.no_grad():
        sr = net(x)
    assert set(net.state_dict().keys()) == set(table(g, "bsrgan_x4_r2_s3/wsum").keys())
    twin = copy.deepcopy(net)
    with torch.no_grad():
        assert torch.equal(twin(x), sr)
    fresh = M.bsrgan_x4(num_rrdb=2).cuda()
    fresh.compute_dtype = torch.float32
    fresh.load_state_dict(net.state_dict())
    with torch.no_grad():
        assert torch.equal(fresh(x), sr)
    assert _rel(sr, g["bsrgan_x4_r2_s3/sr"]) < 1e-3


def test_bf16_gradient_fidelity_23_blocks():
    """The benchmark dtype against the exact-fp32 mode through all 23 RRDBs (351 convs forward, the same backward): the bf16
    flat gradient must point the same way as the f32 one -- cosine similarity, relative norm -- not just be finite."""
    from sr_gan_fd_amd import model as M
    torch.manual_seed(0)
    g = M.bsrgan_x4(in_channels=3, out_channels=3, channels=64, growth_channels=32, num_rrdb=23)
    scaled_init(g, 3.0, 0.5)
    g.cuda().train()
    lr, gt = torch.rand(4, 3, 48, 48, device="cuda"), torch.rand(4, 3, 192, 192, device="cuda")
    grads, losses = {}, {}
    for dt in (torch.float32, torch.bfloat16):
        g.compute_dtype = dt
        g.zero_grad(set_to_none=True)
        loss = F.l1_loss(g(lr), gt)
        loss.backward()
        grads[dt] = torch.cat([p.grad.reshape(-1) for p in g.parameters()]).double()
        losses[dt] = loss.item()
    a, b = grads[torch.float32], grads[torch.bfloat16]
    cos = (a @ b / (a.norm() * b.norm())).item()
    ratio = (b.norm() / a.norm()).item()
    print(f"23-block gradient: bf16 vs f32 cosine {cos:.4f}, norm ratio {ratio:.4f}, loss {losses[torch.bfloat16]:.6f} vs {losses[torch.float32]:.6f}")
    assert cos > 0.98 and 0.9 < ratio < 1.1
    assert abs(losses[torch.bfloat16] - losses[torch.float32]) < 5e-3 * losses[torch.float32]


def test_f16_smooth_loss_gradient_through_23_blocks():
    """The f16 backward pass gated by something other than sign flips: the seed of an L1 loss is +-1/n, so the bounds above measure how
    many pixels change sides.  Here the loss is sum(sr * r) for a fixed smooth r -- the seed is r itself, the same in both modes up to its
    f16 rounding -- through all 23 RRDBs (351 convs, the same number of data- and weight-gradient launches), loss-scaled by 1024 as the
    reference's GradScaler would: the f16 flat gradient against the exact-fp32 mode's at <= 2e-2 relative L2 and cosine >= 0.999."""
    from sr_gan_fd_amd import model as M
    torch.manual_seed(0)
    g = M.bsrgan_x4(in_channels=3, out_channels=3, channels=64, growth_channels=32, num_rrdb=23)
    scaled_init(g, 3.0, 0.5)
    g.cuda().train()
    lr = torch.rand(2, 3, 32, 32, device="cuda")
    yy, xx = torch.meshgrid(torch.linspace(0, 3.1, 128, device="cuda"), torch.linspace(0, 2.3, 128, device="cuda"), indexing="ij")
    r = torch.stack([torch.sin(yy + c) * torch.cos(xx * (c + 1)) for c in range(3)])[None].repeat(2, 1, 1, 1) / (2 * 3 * 128 * 128)
    S = 1024.0
    grads = {}
    for dt in (torch.float32, torch.float16):
        g.compute_dtype = dt
        g.zero_grad(set_to_none=True)
        (g(lr) * (r * S)).sum().backward()
        grads[dt] = torch.cat([p.grad.reshape(-1) for p in g.parameters()]).double() / S
    a, b = grads[torch.float32], grads[torch.float16]
    assert torch.isfinite(b).all()
    cos = (a @ b / (a.norm() * b.norm())).item()
    rel = ((a - b).norm() / a.norm()).item()
    print(f"23-block smooth-loss gradient: f16 vs f32 cosine {cos:.6f}, relative L2 {rel:.3e}")
    assert cos >= 0.999 and rel <= 2e-2


def test_fused_trainer_actually_learns():
    """end-to-end sanity of forward + backward + Adam + EMA in the benchmark dtype: over-fitting one small batch must drive the
    L1 loss down steadily (a wrong-signed or mis-scaled gradient anywhere in the 3-block net would stall or diverge)"""
    from sr_gan_fd_amd import model as M
    from sr_gan_fd_amd.trainer import GeneratorTrainer
    torch.manual_seed(0)
    g = M.bsrgan_x4(in_channels=3, out_channels=3, channels=64, growth_channels=32, num_rrdb=3)
    scaled_init(g, 3.0, 0.5)
    g.compute_dtype = torch.bfloat16
    g.cuda().train()
    tr = GeneratorTrainer(g, lr=1e-3, betas=(0.9, 0.99), eps=1e-4, ema_decay=0.999)
    lr = torch.rand(2, 3, 16, 16, device="cuda")
    gt = F.interpolate(lr, scale_factor=4, mode="bilinear", align_corners=False)      # a learnable target (noise is not)
    losses = [tr.step(lr, gt).item() for _ in range(60)]
    print("over-fit losses:", [round(v, 4) for v in losses[::10]], round(losses[-1], 4))
    assert np.isfinite(losses).all()
    assert losses[-1] < 0.75 * losses[0] and min(losses[-5:]) < min(losses[:5])


def test_reference_amp_wrappers_may_stay():
    """the scripts' ``amp.autocast()`` + ``GradScaler`` (train_bsrnet.py:250-262) wrap the drop-in module
    unchanged -- the scaled loss is back-propagated through the HIP path and unscaled by the scaler; the step must equal the
    plain fp32-loss step."""
    from torch import amp
    from sr_gan_fd_amd import model as M

    def build():
        torch.manual_seed(0)
        g = M.bsrgan_x4(in_channels=3, out_channels=3, channels=64, growth_channels=32, num_rrdb=2)
        scaled_init(g, 3.0, 0.5)
        g.compute_dtype = torch.float32
        return g.cuda().train()
    lr, gt = torch.rand(2, 3, 16, 16, device="cuda"), torch.rand(2, 3, 64, 64, device="cuda")
    a, b = build(), build()
    oa = torch.optim.Adam(a.parameters(), 1e-4, (0.9, 0.99), 1e-4)
    ob = torch.optim.Adam(b.parameters(), 1e-4, (0.9, 0.99), 1e-4)
    scaler = amp.GradScaler("cuda")
    for _ in range(2):
        a.zero_grad(set_to_none=True)
        with amp.autocast("cuda"):
            loss_a = F.l1_loss(a(lr), gt)
        scaler.scale(loss_a).backward()
        scaler.step(oa)
        scaler.update()
        b.zero_grad(set_to_none=True)
        loss_b = F.l1_loss(b(lr), gt)
        loss_b.backward()
        ob.step()
        assert abs(loss_a.item() - loss_b.item()) < 1e-5
    fa = torch.cat([p.detach().reshape(-1) for p in a.parameters()])
    fb = torch.cat([p.detach().reshape(-1) for p in b.parameters()])
    assert ((fa - fb).abs().max() / fb.abs().max()).item() < 1e-5


def test_runs_on_the_callers_stream():
    """Every launch goes to torch's *current* stream (CUDAPrefetcher and user code switch streams): an iteration issued inside
    ``torch.cuda.stream(side)`` right after asynchronous producers on that stream gives the results of the default-stream run, and
    leaves the default stream idle (a kernel enqueued there beforehand is not waited for)."""
    from sr_gan_fd_amd import model as M
    from sr_gan_fd_amd.trainer import GeneratorTrainer

    def build():
        torch.manual_seed(0)
        g = M.bsrgan_x4(num_rrdb=2)
        scaled_init(g, 3.0, 0.5)
        g.compute_dtype = torch.bfloat16
        return g.cuda().train()
    lr0, gt0 = torch.rand(4, 3, 24, 24, device="cuda"), torch.rand(4, 3, 96, 96, device="cuda")
    ref = GeneratorTrainer(build(), lr=1e-4)
    want_loss = [ref.step(lr0, gt0).clone() for _ in range(2)]
    want_flat = ref.opt.flat.clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    tr = GeneratorTrainer(build(), lr=1e-4)
    torch.cuda.synchronize()
    got_loss = []
    with torch.cuda.stream(side):
        lr1 = (lr0 * 2.0) * 0.5                  # producers on the side stream: the step must be ordered after them
        gt1 = (gt0 * 2.0) * 0.5
        for _ in range(2):
            got_loss.append(tr.step(lr1, gt1).clone())
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got_loss, want_loss))
    assert torch.equal(tr.opt.flat, want_flat)


def test_planar_dense_block_buffers_change_nothing_but_the_addresses(monkeypatch):
    """The generator keeps its dense-block buffers as planar 32-channel groups; SRGANFD_PLANAR=0 keeps them NHWC.  Same
    kernels, same summation order: SR, loss and the updated parameters of a training iteration are bitwise equal in both layouts,
    at a size that is not a multiple of the tiles (ragged edges exercise the per-plane row ends)."""
    from sr_gan_fd_amd import model as M
    from sr_gan_fd_amd.trainer import GeneratorTrainer
    lr, gt = torch.rand(3, 3, 37, 52, device="cuda"), torch.rand(3, 3, 148, 208, device="cuda")
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("SRGANFD_PLANAR", flag)
        torch.manual_seed(0)
        g = M.bsrgan_x4(num_rrdb=2)
        scaled_init(g, 3.0, 0.5)
        g.compute_dtype = torch.bfloat16
        tr = GeneratorTrainer(g.cuda().train(), lr=1e-4)
        losses = [tr.step(lr, gt).clone() for _ in range(2)]
        assert tr.eng._last.planar == int(flag)
        res[flag] = (losses, tr.sr.clone(), tr.opt.flat.clone())
    assert all(torch.equal(a, b) for a, b in zip(res["1"][0], res["0"][0]))
    assert torch.equal(res["1"][1], res["0"][1]) and torch.equal(res["1"][2], res["0"][2])


@pytest.mark.parametrize("name,fac,kw,B,h,lr,eps", [
    ("esrgan_small", "rrdbnet_x4", dict(num_blocks=2), 2, 16, 2e-4, 1e-8),        # ESRGAN/rrdbnet_config.py:68-78
    ("bsrnet_small", "bsrgan_x4", dict(num_rrdb=2), 2, 16, 1e-4, 1e-4),           # BSRGAN/bsrnet_config.py:86-96
    ("cfg1_esrgan_b4_32", "rrdbnet_x4", dict(num_blocks=23), 4, 32, 2e-4, 1e-8),  # BASELINE.json configs[0]: batch 4, 32 -> 128, 23 RRDB
])
def test_g_only_steps(golden_dir, name, fac, kw, B, h, lr, eps):
    """trainer.GeneratorTrainer.step == two iterations of ESRGAN/train_rrdbnet.py:244-267 / BSRGAN/train_bsrnet.py:244-272 run on
    the reference's own modules with torch.optim.Adam (g_only_steps.npz): loss, SR and per-tensor parameter checksums after each
    iteration, f32 mode, 1e-3.  The configs[0] inputs are not stored (1.5 MB): they are the next draws of the seeded generator after
    the module's construction, which this repo's module reproduces draw for draw."""
    from sr_gan_fd_amd import model as M
    from sr_gan_fd_amd.trainer import GeneratorTrainer
    g = load_golden(golden_dir, "g_only_steps.npz")
    torch.manual_seed(0)
    net = getattr(M, fac)(in_channels=3, out_channels=3, channels=64, growth_channels=32, **kw)
    scaled_init(net, 3.0, 0.5)
    net.compute_dtype = torch.float32
    stored = f"{name}/it0_lr" in g.files
    draws = [(torch.rand(B, 3, h, h), torch.rand(B, 3, 4 * h, 4 * h)) for _ in range(2)]     # the generator state right after construction
    net.cuda().train()
    tr = GeneratorTrainer(net, lr=lr, betas=(0.9, 0.99), eps=eps, ema_decay=None)
    for it in range(2):
        x, gt = draws[it]
        if stored:
            assert torch.equal(x, torch.tensor(g[f"{name}/it{it}_lr"])) and torch.equal(gt, torch.tensor(g[f"{name}/it{it}_gt"]))
        loss = tr.step(x.cuda(), gt.cuda()).item()
        want = float(g[f"{name}/losses"][it])
        print(f"{name} it{it}: loss {loss:.7f} (reference {want:.7f})")
        assert abs(loss - want) < 1e-3 * abs(want)
        if stored:
            assert _rel(tr.sr, g[f"{name}/it{it}_sr"]) < 1e-3
        sd = net.state_dict()
        # Adam's first steps move every element by ~lr * g / (|g| + eps): with eps = 1e-8 an element whose gradient is within fp32
        # summation-order noise of zero (|g| ~ 1e-8: zero-initialised biases deep in the trunk) lands anywhere in [-lr, +lr], in the
        # reference's own arithmetic as much as here.  The checksums therefore get an absolute slack of two such elements on top of
        # the 2e-3 relative bound; everything else (loss, SR, the eps = 1e-4 case) is held to 1e-3 / 2e-3.
        slack = 4.0 * lr if eps < 1e-6 else 0.0
        for k, want_c in table(g, f"{name}/it{it}_wsum").items():
            assert np.allclose(checksum(sd[k]), want_c, rtol=2e-3, atol=2e-4 * abs(want_c[1]) + slack), f"{name} it{it} {k}: {checksum(sd[k])} vs {want_c}"
    assert _rel(net.conv4.bias, g[f"{name}/conv4_bias"]) < 1e-3


def test_packed_weights_follow_updates_in_every_dtype():
    """Each compute dtype keeps its own packed copy of the weights; after a fused optimizer step EVERY copy is stale, not only the
    one of the dtype that runs next (a shared 'seen' marker let a bf16 forward run on pre-step weights after an f32 forward
    had consumed the change)."""
    from sr_gan_fd_amd import model as M
    from sr_gan_fd_amd.trainer import GeneratorTrainer
    torch.manual_seed(0)
    net = M.bsrgan_x4(num_rrdb=1)
    scaled_init(net, 3.0, 0.5)
    net.cuda().train()
    x, gt = torch.rand(1, 3, 16, 16).cuda(), torch.rand(1, 3, 64, 64).cuda()

    def fwd(dt):
        net.compute_dtype = dt
        with torch.no_grad():
            return net(x).clone()
    b0, f0 = fwd(torch.bfloat16), fwd(torch.float32)
    net.compute_dtype = torch.float32
    tr = GeneratorTrainer(net, lr=5e-2, betas=(0.9, 0.99), eps=1e-8, ema_decay=None)     # a step large enough to move SR visibly
    tr.step(x, gt)
    f1 = fwd(torch.float32)          # consumes the change for the f32 pack ...
    b1 = fwd(torch.bfloat16)         # ... the bf16 pack must notice it too
    moved = (f1 - f0).abs().max().item()
    assert moved > 5e-2, moved
    assert (b1 - f1).abs().max().item() < 0.25 * moved, "bf16 forward ran on weights from before the optimizer step"
    assert (b1 - b0).abs().max().item() > 0.5 * moved
