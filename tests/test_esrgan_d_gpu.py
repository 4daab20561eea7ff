"""GPU parity of ESRGAN's BatchNorm discriminator against vectors captured from the reference
(ESRGAN/model.py:88-141), and of its backward pass and the differentiable VGG content loss's against a float64 oracle that rounds where
the engines store 16-bit values and replays the discrete states their plans stored (tests/esrgan_d_oracle.py; the sharp 16-bit checks,
test_discriminator_matches_oracle and test_content_loss_gradient_matches_oracle)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import esrgan_d_oracle as EO
from tests.util import checksum, load_golden, rounded_weights, table

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a = a.detach().double().cpu() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a)).double()
    b = b.detach().double().cpu() if torch.is_tensor(b) else torch.as_tensor(np.asarray(b)).double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def _build():
    from sr_gan_fd_amd import model as M
    torch.manual_seed(0)
    d = M.discriminator()
    with torch.no_grad():
        for m in d.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.3, 0.3)
    return d


def _rel_l2(a, b):
    a = a.detach().double().cpu() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a)).double()
    b = b.detach().double().cpu() if torch.is_tensor(b) else torch.as_tensor(np.asarray(b)).double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@pytest.mark.parametrize("c", [64, 512])
def test_batchnorm_leakyrelu_fused(c):
    """srganfd_batchnorm_act_fwd / _bwd (BatchNorm2d + LeakyReLU(0.2), channel blocks of 256) vs torch on the same data"""
    from sr_gan_fd_amd import _abi as A
    torch.manual_seed(2)
    n, h, w = 4, 8, 12
    L, st = A.lib(), A.stream_ptr()
    bn = torch.nn.BatchNorm2d(c)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
    x = (torch.randn(n, c, h, w) * 2 + 1).requires_grad_(True)
    y = F.leaky_relu(bn(x), 0.2)
    dy = torch.randn_like(y)
    y.backward(dy)
    xa = x.detach().permute(0, 2, 3, 1).contiguous().cuda()
    ya, dxa = torch.empty_like(xa), torch.empty_like(xa)
    rm, rv = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
    save, ws = torch.empty(4 * c, device="cuda"), torch.empty(2048 * 256 + 768, device="cuda")
    gam, bet = bn.weight.detach().cuda(), bn.bias.detach().cuda()
    A.check(L.srganfd_batchnorm_act_fwd(A.view(xa), A.view(ya), A.F32, n * h * w, c, gam.data_ptr(), bet.data_ptr(), rm.data_ptr(), rv.data_ptr(),
                                        0.1, 1e-5, 1, save.data_ptr(), ws.data_ptr(), 0.2, st))
    dg, db = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
    dya = dy.permute(0, 2, 3, 1).contiguous().cuda()
    A.check(L.srganfd_batchnorm_act_bwd(A.view(xa), A.view(dya), A.view(dxa), A.F32, n * h * w, c, gam.data_ptr(), save.data_ptr(), dg.data_ptr(),
                                        db.data_ptr(), 0.0, ws.data_ptr(), A.view(ya), 0.2, st))
    torch.cuda.synchronize()
    assert _rel(ya.permute(0, 3, 1, 2), y) < 1e-5
    assert _rel(rm, bn.running_mean) < 1e-5 and _rel(rv, bn.running_var) < 1e-5
    assert _rel(dxa.permute(0, 3, 1, 2), x.grad) < 1e-4
    assert _rel(dg, bn.weight.grad) < 1e-4 and _rel(db, bn.bias.grad) < 1e-4


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_esrgan_discriminator(golden_dir, dtype):
    """Pins the engine to the reference's own vectors (tests/golden/esrgan_discriminator.npz): two training forwards, the loss, sampled
    gradients, eval mode, the input gradient of a frozen pass.  Its 16-bit gradient bounds are hand-set and loose (a wrong LeakyReLU'
    slope or BatchNorm backward in one stage passes them, tests/test_esrgan_d_host.py): the sharp check of the backward pass is
    test_discriminator_matches_oracle below."""
    g = load_golden(golden_dir, "esrgan_discriminator.npz")
    f32 = dtype == torch.float32
    # 16-bit bounds per dtype (measured f16 / bf16: logits 1.8e-3 / 4.1e-2; sampled weight gradients, relative L2, worst 1.2e-1 / 2.5e-1 --
    # LeakyReLU masks of values within one 16-bit rounding of zero flip, each flip changes that element's gradient 5x; input gradient
    # 1.1e-1 / 2.2e-1): f16 is the benchmarked dtype and gets its own, tighter, numbers
    B16 = {torch.float16: dict(logits=5e-3, state=5e-3, loss=5e-3, grad=1.8e-1, dx=1.6e-1),
           torch.bfloat16: dict(logits=6e-2, state=3e-2, loss=5e-2, grad=3e-1, dx=3e-1)}.get(dtype)
    d = _build()
    d.compute_dtype = dtype
    d.cuda().train()
    x = torch.tensor(g["x"]).cuda()
    for it in range(2):
        logits = d(x)
        e = _rel(logits, g[f"train{it}_logits"])
        print(f"ESRGAN D {dtype} train fwd {it}: logits err {e:.2e}")
        assert e < (1e-3 if f32 else B16["logits"])
        sd = d.state_dict()
        for k, want in table(g, f"train{it}_statesum").items():
            tol = 1e-3 if f32 else B16["state"]
            assert np.allclose(checksum(sd[k]), want, rtol=tol, atol=tol * abs(want[1]) + 1e-7), f"state {k}: {checksum(sd[k])} vs {want}"
    assert int(d.features[3].num_batches_tracked) == 2
    loss = F.binary_cross_entropy_with_logits(logits, torch.ones_like(logits))
    assert abs(loss.item() - float(g["bce_ones"])) < (1e-3 if f32 else B16["loss"])
    S = 65536.0 if dtype == torch.float16 else 1.0       # f16 backward runs loss-scaled, as under the reference's GradScaler
    (loss * S).backward()
    named = dict(d.named_parameters())
    for p in named.values():
        p.grad /= S
    # The stack is conv -> BatchNorm -> LeakyReLU nine times: normalised values sit densely around zero, so a conv output
    # that differs from the reference's by fp32 summation order (~5e-6 here) flips a few dozen LeakyReLU masks in the
    # large early maps; each flip changes one element's gradient 5x and, through BatchNorm's channel sums, nudges its
    # whole channel.  (Measured: stage-9 gradients agree to 2e-6, one flipped element of 131072 in stage 8; the fused
    # BatchNorm+LeakyReLU kernels themselves are checked to 1e-4 above.)  Hence L2 bounds, looser towards the input.
    worst = 0.0
    for key in g.files:
        if key.startswith("grad/"):
            e = _rel_l2(named[key[5:]].grad, g[key])
        elif key.startswith("gradrows/"):
            e = _rel_l2(named[key[9:]].grad[:2], g[key])
        else:
            continue
        worst = max(worst, e)
        print(f"  {key}: L2 err {e:.2e}")
        deep = any(t in key for t in ("features.26", "features.27", "classifier"))
        assert e < ((1e-4 if deep else 2e-2) if f32 else B16["grad"]), f"{key}: {e:.2e}"
    print(f"ESRGAN D {dtype}: worst sampled grad L2 err {worst:.2e}")
    if f32:
        for k, want in table(g, "gsum").items():
            got = checksum(named[k].grad)
            assert np.allclose(got, want, rtol=2e-2, atol=5e-3 * abs(want[1]) + 1e-6), f"grad checksum {k}: {got} vs {want}"
    d.eval()
    with torch.no_grad():
        assert _rel(d(x), g["eval_logits"]) < (1e-3 if f32 else B16["logits"])
    d.train()
    for p in d.parameters():
        p.requires_grad = False
    xin = x.clone().requires_grad_(True)
    lg = d(xin)
    assert _rel(lg, g["train2_logits"]) < (1e-3 if f32 else B16["logits"])
    (F.binary_cross_entropy_with_logits(lg, torch.ones_like(lg)) * S).backward()
    ref = torch.tensor(g["train2_dx"]).double()
    e2 = ((xin.grad.double().cpu() / S - ref).norm() / ref.norm()).item()
    print(f"ESRGAN D {dtype}: input-gradient L2 err {e2:.2e}")
    assert e2 < (3e-2 if f32 else B16["dx"])


F16_GRAD_L2 = 1.5e-1      # d/dSR of the single-node content loss in f16 vs the f16-weight oracle, relative L2 (sign flips of |sr_f - gt_f| ~ f16 error)
# (hand-set and loose; the sharp check of d/dSR, with the flipped states replayed, is test_content_loss_gradient_matches_oracle below)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_differentiable_single_node_content_loss(dtype):
    """ESRGAN ContentLoss (one node, kept in the autograd graph: ESRGAN/model.py:258-292): value and d/dSR vs the CPU oracle
    (seeded VGG-19 weights: the ImageNet file is a network download, parity of VALUES stays unpinned as for BSRGAN's).
    Asserted: value 1e-4 (f32), 2e-3 (f16, oracle on the same f16-rounded conv weights), 3e-2 (bf16); d/dSR L2 1e-2 / F16_GRAD_L2 / 4e-1."""
    from oracle import srgan_oracle as O
    from sr_gan_fd_amd import model as M
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    cl = M.ContentLoss("features.34", mean, std)
    cl.compute_dtype = dtype
    cl.cuda()
    torch.manual_seed(3)
    sr, gt = torch.rand(2, 3, 48, 32), torch.rand(2, 3, 48, 32)
    s = sr.clone().cuda().requires_grad_(True)
    loss = cl(s, gt.cuda())
    (2.5 * loss).backward()
    P = {"features." + k: v.detach().cpu() for k, v in cl.features.state_dict().items()}
    if dtype == torch.float16:
        P = rounded_weights(P, dtype)
    so = sr.clone().requires_grad_(True)
    want = O.content_loss_single(so, gt, P, "features.34", mean, std)
    (2.5 * want).backward()
    f32 = dtype == torch.float32
    e_l = abs(loss.item() - want.item()) / abs(want.item())
    e_g = _rel_l2(s.grad, so.grad)
    print(f"single-node content loss {dtype}: value {loss.item():.6f} vs {want.item():.6f} (rel {e_l:.2e}), dSR L2 err {e_g:.2e}, max {_rel(s.grad, so.grad):.2e}")
    assert loss.dim() == 0 and e_l < {torch.float32: 1e-4, torch.float16: 2e-3, torch.bfloat16: 3e-2}[dtype]
    # L2 bound: ~1M ReLU inputs, fp32 conv outputs that differ from the reference's by summation order (~5e-6) -> a handful
    # of mask flips, each worth sqrt(1/#active) of a layer's gradient (the oracle in fp64 vs fp32 shows none: 6e-7)
    # bf16: the tap gradient is sign(sr_f - gt_f); wherever |sr_f - gt_f| is below the bf16 error of 16 chained convs the sign
    # flips outright, so the bf16 gradient is only loosely tied to the fp32 one (the reference's fp16 autocast has the same trait)
    # f16 (11 bits): the same trait, an order of magnitude weaker
    assert e_g < {torch.float32: 1e-2, torch.float16: F16_GRAD_L2, torch.bfloat16: 4e-1}[dtype]
    with torch.no_grad():
        assert abs(cl(sr.cuda(), gt.cuda()).item() - loss.item()) < 1e-6 * abs(loss.item()) + 1e-9


def test_maxpool_relu_backward_and_l1_sign_kernels():
    from sr_gan_fd_amd import _abi as A
    torch.manual_seed(4)
    n, c, h, w = 2, 32, 8, 12
    L, st = A.lib(), A.stream_ptr()
    z = torch.randn(n, c, h, w, requires_grad=True)
    y = F.max_pool2d(F.relu(z), 2, 2)
    dy = torch.randn_like(y)
    y.backward(dy)
    xa = F.relu(z).detach().permute(0, 2, 3, 1).contiguous().cuda()
    dya = dy.permute(0, 2, 3, 1).contiguous().cuda()
    dxa = torch.empty_like(xa)
    A.check(L.srganfd_maxpool2_relu_bwd(A.view(xa), A.view(dya), A.view(dxa), A.F32, n, h, w, c, st))
    a, b = torch.randn(n, h, w, c, device="cuda"), torch.randn(n, h, w, c, device="cuda")
    b[0, 0, 0, :4] = a[0, 0, 0, :4]                        # exact ties: sign(0) = 0
    up = torch.tensor([1.5], device="cuda")
    out = torch.empty_like(a)
    A.check(L.srganfd_l1_grad_views(A.view(a), A.view(b), A.view(out), A.F32, n * h * w, c, up.data_ptr(), 0.25, st))
    torch.cuda.synchronize()
    assert torch.equal(dxa.permute(0, 3, 1, 2).cpu(), z.grad)
    assert torch.equal(out, 0.375 * torch.sign(a - b))


def test_esrgan_relativistic_iterations_on_dropin_modules(golden_dir):
    """The reference's own loop body (ESRGAN/train_esrgan.py:364-431: torch.optim.Adam, BCEWithLogitsLoss, L1Loss, autograd
    with retain_graph and three live discriminator forwards) over the drop-in RRDBNet / Discriminator modules."""
    from sr_gan_fd_amd import model as M
    from tests.util import scaled_init
    g = load_golden(golden_dir, "esrgan_gan_steps.npz")
    torch.manual_seed(0)
    d = M.discriminator()
    gen = M.rrdbnet_x4(in_channels=3, out_channels=3, channels=64, growth_channels=32, num_blocks=2)
    scaled_init(gen, 3.0, 0.5)
    d.compute_dtype = gen.compute_dtype = torch.float32
    d.cuda().train()
    gen.cuda().train()
    d_opt = torch.optim.Adam(d.parameters(), 1e-4, (0.9, 0.99), 1e-8, 0.0)
    g_opt = torch.optim.Adam(gen.parameters(), 1e-4, (0.9, 0.99), 1e-8, 0.0)
    bce, l1 = torch.nn.BCEWithLogitsLoss(), torch.nn.L1Loss()
    for it in range(2):
        lr, gt = torch.tensor(g[f"it{it}_lr"]).cuda(), torch.tensor(g[f"it{it}_gt"]).cuda()
        B = gt.shape[0]
        real, fake = torch.full([B, 1], 1.0, device="cuda"), torch.full([B, 1], 0.0, device="cuda")
        for p in d.parameters():
            p.requires_grad = False
        gen.zero_grad(set_to_none=True)
        sr = gen(lr)
        gt_output = d(gt.detach().clone())
        sr_output = d(sr)
        pixel = 0.01 * l1(sr, gt)
        adv = 0.005 * (bce(gt_output - torch.mean(sr_output), fake) * 0.5 + bce(sr_output - torch.mean(gt_output), real) * 0.5)
        (pixel + adv).backward()
        g_opt.step()
        for p in d.parameters():
            p.requires_grad = True
        d.zero_grad(set_to_none=True)
        gt_output = d(gt)
        sr_output = d(sr.detach().clone())
        d_loss_gt = bce(gt_output - torch.mean(sr_output), real) * 0.5
        d_loss_gt.backward(retain_graph=True)
        sr_output = d(sr.detach().clone())
        d_loss_sr = bce(sr_output - torch.mean(gt_output), fake) * 0.5
        d_loss_sr.backward()
        d_opt.step()
        got = [(d_loss_gt + d_loss_sr).item(), pixel.item(), adv.item(), torch.sigmoid(torch.mean(gt_output.detach())).item(),
               torch.sigmoid(torch.mean(sr_output.detach())).item()]
        want = g[f"it{it}_scalars"]
        print(f"ESRGAN relativistic it{it}: got {got} want {list(want)}")
        # iteration 1 starts from parameters that already took sign-like Adam steps (eps 1e-8): see the oracle test's note
        assert np.allclose(got, want, rtol=1e-3 if it == 0 else 2e-2, atol=1e-5)
        assert _rel(sr[:, :, ::4, ::4], g[f"it{it}_sr"]) < (1e-3 if it == 0 else 2e-2)
    assert int(d.features[3].num_batches_tracked) == 10          # five training forwards per iteration


def _esrgan_pair(dtype):
    from sr_gan_fd_amd import model as M
    from tests.util import scaled_init
    torch.manual_seed(0)
    d = M.discriminator()
    gen = M.rrdbnet_x4(in_channels=3, out_channels=3, channels=64, growth_channels=32, num_blocks=2)
    scaled_init(gen, 3.0, 0.5)
    d.compute_dtype = gen.compute_dtype = dtype
    return gen.cuda().train(), d.cuda().train()


def test_esrgan_fused_relativistic_trainer_vs_reference(golden_dir):
    """EsrganGanTrainer.step == two iterations of ESRGAN/train_esrgan.py:340-431 run on the reference's own modules (esrgan_gan_steps.npz:
    generator first, relativistic-average losses, five BatchNorm-advancing discriminator forwards, Adam, EMA; content loss stubbed to 0):
    logged scalars, SR, every parameter's checksum after both optimizer steps.  Iteration 1 starts from parameters that took sign-like
    Adam steps (eps 1e-8), hence its looser bound -- the same the module-level loop above and the CPU oracle meet."""
    from sr_gan_fd_amd.gan_esrgan import EsrganGanTrainer
    from tests.util import checksum, table
    g = load_golden(golden_dir, "esrgan_gan_steps.npz")
    gen, d = _esrgan_pair(torch.float32)
    tr = EsrganGanTrainer(gen, d, None)
    for it in range(2):
        s = tr.step(torch.tensor(g[f"it{it}_lr"]).cuda(), torch.tensor(g[f"it{it}_gt"]).cuda()).cpu().numpy()
        want = g[f"it{it}_scalars"]                     # d_loss, pixel, adversarial, sigmoid(mean D(gt)), sigmoid(mean D(sr))
        got = [s[0], s[1], s[3], s[4], s[5]]
        print(f"ESRGAN fused it{it}: got {got} want {list(want)}")
        tol = 1e-3 if it == 0 else 2e-2
        assert np.allclose(got, want, rtol=tol, atol=1e-5)
        assert _rel(tr.sr[:, :, ::4, ::4], g[f"it{it}_sr"]) < tol
        if it == 0:
            for sd, key in ((gen.state_dict(), "it0_wsum_g"), (d.state_dict(), "it0_wsum_d")):
                for k, want_c in table(g, key).items():
                    if "num_batches_tracked" in k:
                        assert int(sd[k]) == int(want_c[0]), k
                    else:
                        # Adam with eps 1e-8 moves every element by ~lr * sign(g) = 1e-4: an element whose gradient is within rounding of
                        # zero lands on the other side (2e-4 in a checksum).  Bound: 5e-3 of the tensor's absolute sum, or four such flips
                        # (the 32- / 64-element biases start at zero, so their whole content is this step)
                        assert np.allclose(checksum(sd[k]), want_c, rtol=5e-3, atol=max(5e-3 * abs(want_c[1]), 8e-4)), f"{key} {k}"
    assert int(d.features[3].num_batches_tracked) == 10          # five training forwards per iteration


def test_esrgan_fused_trainer_matches_module_level_loop_with_content_loss():
    """With the differentiable single-node VGG content loss switched on (seeded random extractor: the ImageNet weights are not in the
    reference tree), the fused trainer and the script's own autograd loop over the drop-in modules take the same two steps."""
    from sr_gan_fd_amd import model as M
    from sr_gan_fd_amd.gan_esrgan import EsrganGanTrainer
    MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    data = []
    torch.manual_seed(7)
    for _ in range(2):
        data.append((torch.rand(2, 3, 32, 32).cuda(), torch.rand(2, 3, 128, 128).cuda()))
    # fused
    gen, d = _esrgan_pair(torch.float32)
    torch.manual_seed(1)
    cl = M.content_loss("features.34", MEAN, STD)
    cl.compute_dtype = torch.float32
    cl.cuda()
    tr = EsrganGanTrainer(gen, d, cl, ema_decay=None)
    fused = [tr.step(lr, gt).cpu().numpy().copy() for lr, gt in data]
    # the script's loop on the modules (torch.optim.Adam, autograd)
    gen2, d2 = _esrgan_pair(torch.float32)
    torch.manual_seed(1)
    cl2 = M.content_loss("features.34", MEAN, STD)
    cl2.compute_dtype = torch.float32
    cl2.cuda()
    d_opt = torch.optim.Adam(d2.parameters(), 1e-4, (0.9, 0.99), 1e-8, 0.0)
    g_opt = torch.optim.Adam(gen2.parameters(), 1e-4, (0.9, 0.99), 1e-8, 0.0)
    bce, l1 = torch.nn.BCEWithLogitsLoss(), torch.nn.L1Loss()
    for it, (lr, gt) in enumerate(data):
        B = gt.shape[0]
        real, fake = torch.full([B, 1], 1.0, device="cuda"), torch.full([B, 1], 0.0, device="cuda")
        for p in d2.parameters():
            p.requires_grad = False
        gen2.zero_grad(set_to_none=True)
        sr = gen2(lr)
        gt_output = d2(gt.detach().clone())
        sr_output = d2(sr)
        pixel, content = 0.01 * l1(sr, gt), 1.0 * cl2(sr, gt)
        adv = 0.005 * (bce(gt_output - torch.mean(sr_output), fake) * 0.5 + bce(sr_output - torch.mean(gt_output), real) * 0.5)
        (pixel + content + adv).backward()
        g_opt.step()
        for p in d2.parameters():
            p.requires_grad = True
        d2.zero_grad(set_to_none=True)
        gt_output = d2(gt)
        sr_output = d2(sr.detach().clone())
        d_loss_gt = bce(gt_output - torch.mean(sr_output), real) * 0.5
        d_loss_gt.backward(retain_graph=True)
        sr_output = d2(sr.detach().clone())
        d_loss_sr = bce(sr_output - torch.mean(gt_output), fake) * 0.5
        d_loss_sr.backward()
        d_opt.step()
        want = [(d_loss_gt + d_loss_sr).item(), pixel.item(), content.item(), adv.item(), torch.sigmoid(torch.mean(gt_output.detach())).item(),
                torch.sigmoid(torch.mean(sr_output.detach())).item()]
        print(f"it{it}: fused {list(fused[it][:6])} loop {want}")
        assert np.allclose(fused[it][:6], want, rtol=1e-3 if it == 0 else 2e-2, atol=1e-5)
    assert _rel(gen.conv1.weight, gen2.conv1.weight) < 2e-2 and _rel(d.classifier[2].weight, d2.classifier[2].weight) < 2e-2


def test_esrgan_fused_trainer_f16_stays_close_to_f32():
    """The benchmark dtype: f16 activations / loss-scaled gradients against the f32 run of the same two iterations -- scalars within 5e-3
    relative (BatchNorm statistics over 2 images at 128x128 amplify one f16 rounding of the logits), no skipped optimizer step."""
    from sr_gan_fd_amd.gan_esrgan import EsrganGanTrainer
    torch.manual_seed(11)
    data = [(torch.rand(2, 3, 32, 32).cuda(), torch.rand(2, 3, 128, 128).cuda()) for _ in range(2)]
    outs = {}
    for dt in (torch.float32, torch.float16):
        gen, d = _esrgan_pair(dt)
        tr = EsrganGanTrainer(gen, d, None)
        outs[dt] = np.stack([tr.step(lr, gt).cpu().numpy()[:6].copy() for lr, gt in data])
        if dt == torch.float16:
            rep = tr.scaler.report()
            assert rep["enabled"] and rep["optimizer_steps"] == 4 and rep["skipped"] == 0, rep
    a, b = outs[torch.float32][0], outs[torch.float16][0]
    err = np.abs(a - b) / np.maximum(np.abs(a), 1e-6)
    print("f32", a, "f16", b, "rel", err)
    assert err[[0, 1, 3, 4, 5]].max() < 5e-3


def test_esrgan_fused_trainer_checkpoint_resume_is_bitwise():
    """EsrganGanTrainer.state_dict() / load_state_dict() (ESRGAN/train_esrgan.py:216-262 checkpoints g, d, both optimizers and the EMA
    model every epoch and resumes from them): a trainer rebuilt from fresh modules + the checkpoint takes bitwise the same third
    iteration as the one that kept running -- weights, BatchNorm running statistics, Adam moments and step, EMA, loss scale."""
    from sr_gan_fd_amd.gan_esrgan import EsrganGanTrainer
    torch.manual_seed(11)
    data = [(torch.rand(2, 3, 32, 32).cuda(), torch.rand(2, 3, 128, 128).cuda()) for _ in range(3)]
    gen, d = _esrgan_pair(torch.float16)
    tr = EsrganGanTrainer(gen, d, None)
    for lr, gt in data[:2]:
        tr.step(lr, gt)
    ckpt = tr.state_dict()
    assert set(ckpt) == {"g", "d", "scaler"} and set(ckpt["g"]) == {"state_dict", "optimizer", "ema_state_dict"}
    assert int(ckpt["g"]["ema_state_dict"]["n_averaged"]) == 2 and len(ckpt["d"]["optimizer"]["state"]) == len(list(d.parameters()))
    ckpt = {k: ({kk: (vv if not torch.is_tensor(vv) else vv.clone()) for kk, vv in v.items()} if k != "scaler" else dict(v)) for k, v in ckpt.items()}
    ckpt["g"]["state_dict"] = {k: v.clone() for k, v in ckpt["g"]["state_dict"].items()}
    ckpt["d"]["state_dict"] = {k: v.clone() for k, v in ckpt["d"]["state_dict"].items()}
    ckpt["scaler"]["scale"] = 4096.0                       # a value the fresh trainer would not start with
    tr.scaler.scale = 4096.0
    gen2, d2 = _esrgan_pair(torch.float16)
    with torch.no_grad():
        for p in list(gen2.parameters()) + list(d2.parameters()):
            p.add_(0.01)                                   # the checkpoint, not the seed, must provide the weights
    tr2 = EsrganGanTrainer(gen2, d2, None)
    tr2.load_state_dict(ckpt)
    assert tr2.scaler.scale == 4096.0 and tr2.g_opt.n_averaged == 2
    a = tr.step(*data[2]).clone()
    b = tr2.step(*data[2]).clone()
    assert torch.equal(a, b)
    assert torch.equal(tr.g_opt.flat, tr2.g_opt.flat) and torch.equal(tr.d_opt.flat, tr2.d_opt.flat)
    assert torch.equal(tr.g_opt.ema, tr2.g_opt.ema) and torch.equal(tr.g_opt.m, tr2.g_opt.m) and torch.equal(tr.d_opt.v, tr2.d_opt.v)
    for (k, x), (_, y) in zip(d.state_dict().items(), d2.state_dict().items()):
        assert torch.equal(x, y), k


def test_esrgan_iteration_at_the_config_crop_f16_vs_oracle():
    """esrgan_config.py:73-74: x4, LR crops of 32 x 32 (GT 128 x 128 -- the size the BatchNorm discriminator's classifier fixes), the
    23-RRDB generator.  One relativistic GAN iteration (train_esrgan.py:364-431, content term off) of the fused trainer in float16 -- the
    scripts' autocast dtype -- against the fp32 CPU oracle; batch 4 instead of 16 keeps the oracle at seconds.  The generator's dense
    blocks run through the dense-block launch (8 x 16 tiles) in both of its passes.  Asserted: pixel loss within 1e-3 relative
    (BASELINE.json's tolerance); the discriminator-side scalars within 5e-3 (the bound of the f16-against-f32 test above: BatchNorm
    statistics over four images amplify one f16 rounding of the logits); SR within 1e-3."""
    from oracle import srgan_oracle as O
    from sr_gan_fd_amd import model as M, ops
    from sr_gan_fd_amd.gan_esrgan import EsrganGanTrainer
    from tests.util import scaled_init, sd_to_params
    torch.manual_seed(9)
    lr_img, gt = torch.rand(4, 3, 32, 32), torch.rand(4, 3, 128, 128)
    torch.manual_seed(0)
    d = M.discriminator()
    gen = M.rrdbnet_x4(in_channels=3, out_channels=3, channels=64, growth_channels=32, num_blocks=23)
    scaled_init(gen, 3.0, 0.5)
    G = sd_to_params(gen.state_dict())
    D = {k: v.detach().clone() for k, v in d.state_dict().items()}
    g_opt = O.AdamState(G, O.g_param_names(G))
    d_opt = O.AdamState(D, [k for k in D if k.endswith((".weight", ".bias"))])
    out = O.esrgan_gan_step(G, D, g_opt, d_opt, lr_img, gt)
    d.compute_dtype = gen.compute_dtype = torch.float16
    gen, d = gen.cuda().train(), d.cuda().train()
    tr = EsrganGanTrainer(gen, d, None)
    s = tr.step(lr_img.cuda(), gt.cuda()).cpu().numpy()
    sp = tr.ge._last
    n_chain = len([it for it in sp.fw + sp.bw if it.kind == "chain"])
    assert n_chain == 6 * 23 or ops.DENSE_CHAIN == "0", n_chain
    got = [s[0], s[1], s[3], s[4], s[5]]
    want = [out[k] for k in ("d_loss", "pixel_loss", "adversarial_loss", "d_gt_probability", "d_sr_probability")]
    rel = [abs(a - b) / max(abs(b), 1e-6) for a, b in zip(got, want)]
    e_sr = _rel(tr.sr, out["sr"])
    print(f"f16 ESRGAN iteration at 32 -> 128, 23 RRDB: got {got} want {want} rel {[f'{r:.1e}' for r in rel]}; SR {e_sr:.2e}")
    assert rel[1] < 1e-3 and max(rel) < 5e-3 and e_sr < 1e-3
    rep = tr.scaler.report()
    assert rep["optimizer_steps"] == 2 and rep["skipped"] == 0, rep


# ---- the sharp 16-bit checks: both backward passes against the float64 oracle (tests/esrgan_d_oracle.py) ----
MODES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
# The rule needs a tensor: E and G are norms over many elements, each a draw of the rounding noise, and the GPU run's error is another
# draw of the same noise (its fp32 sums run in another order, so values at a rounding boundary fall the other way and the runs drift apart
# like two seeds).  For a tensor of one or two elements -- the two logits at N = 2, classifier.2.bias's one gradient, the content loss --
# E and G are one or two signed draws, by chance anything down to zero: in f16 the emulated oracle's logits differ from the float64
# ones by 2.8e-3 and the GPU's by 7.9e-3, each from stored f1 tensors that meet the rule at 0.5.  Such a tensor is held to the rule
# with a floor, never a wider factor: what the rule's bound on the tensor it is computed FROM allows it (FLOORS below, each with its
# inequality; tests/test_bsrgantrans_gpu.py's l1_floor), and 2 unit roundoffs of fp32 for ONE number (one for the rounding of the kernel's
# result, one for the float32 oracle's: that file's SCALAR_FLOOR).
SCALAR_FLOOR = 2 * 2.0 ** -24
FLIP_FACTOR = 8           # a state may differ from the float64 run's only within FLIP_FACTOR x the oracle's own deviation at that layer


def flip_cap(own, units):
    """tests/test_bsrgantrans_gpu.flip_cap: the emulated oracle's own share, three standard deviations of a count of that size, 8 units"""
    return own + 3 * (own / units) ** 0.5 + 8 / units


def _rule(tag, mode, got, runs, keys, floors=None):
    """prints every err / bound ratio of the rule -- f32: 8 G; 16-bit: max(2 E, 8 G) -- and returns the tensors that miss it.  ``floors``:
    key -> function of the bounds so far (``keys`` is in the order of computation), for the tensors of one or two elements"""
    ref, bad, ratios, bounds = runs["f64"], [], [], {}
    for k in keys:
        want = ref[k].double()
        have = torch.as_tensor(got[k]).detach().double().cpu().reshape(want.shape)
        err, G = EO.rel_l2(have, want), EO.rel_l2(runs["f32"][k], want)
        bound, what = (8 * G, "8G") if mode == "f32" else (max(2 * EO.rel_l2(runs[mode][k], want), 8 * G), "max(2E, 8G)")
        if floors and k in floors:
            assert want.numel() <= 2, k
            floor = max(float(floors[k](bounds)), SCALAR_FLOOR if want.numel() == 1 else 0.0)
            if floor > bound:
                bound, what = floor, "floor (rule: %.3e)" % bound
        bounds[k] = bound
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        ratios.append(ratio)
        print("%-12s %-4s %-44s err %.3e  %s %.3e  ratio %.3f" % (tag, mode, k, err, what, bound, ratio))
        if not err <= bound:
            bad.append((k, err, bound))
    print("%-12s %-4s err / bound over %d tensors: %.3f .. %.3f" % (tag, mode, len(ratios), min(ratios), max(ratios)))
    return bad


def _flips(tag, mode, what, mine, state64, own, margin64, dev):
    """One kind of discrete state at one layer.  ``mine``: the GPU run's; ``state64``: the float64 oracle's; ``own``: the oracle's at the
    mode's precision; ``margin64``: how far each unit of the float64 run is from changing state; ``dev``: the largest deviation, at that
    layer, of the oracle at the mode's precision from the float64 run, in the margin's units.  No unit farther than FLIP_FACTOR x dev from
    the switch may differ.  Returns (flipped, the oracle's own flipped, units, the factor that would have been needed)."""
    flipped = mine != state64
    T = FLIP_FACTOR * dev
    far = flipped & (margin64 > T)
    need = float(margin64[flipped].max() / dev) if bool(flipped.any()) and dev > 0 else 0.0
    assert not bool(far.any()), "%s %s %s: %d units flipped beyond %d x the oracle's deviation %.3e (needed factor %.2f)" % (
        tag, mode, what, int(far.sum()), FLIP_FACTOR, dev, need)
    return int(flipped.sum()), int((own != state64).sum()), flipped.numel(), need


def _share_check(tag, mode, what, rows):
    """the share of flipped states over the layers ``rows`` (of _flips) against its cap"""
    flipped, own, units = [sum(r[i] for r in rows) for i in range(3)]
    need = max(r[3] for r in rows)
    cap = flip_cap(own / units, units)
    print("%-12s %-4s %-14s states that differ from the float64 oracle's: %.2e of %d (the oracle's own at this precision %.2e, cap %.2e); "
          "farthest flipped unit at %.2f x the oracle's deviation (allowed %d)" % (tag, mode, what, flipped / units, units, own / units, cap, need, FLIP_FACTOR))
    if mode != "f32":
        assert flipped / units <= cap, (what, flipped / units, cap)


@functools.lru_cache(maxsize=None)
def _d_pass(mode):
    """three passes of the module on the GPU (full; full again; parameters frozen), what the first one's plan stored, and the oracle's
    runs with the stored signs replayed -- computed once per mode, shared, never written to"""
    from sr_gan_fd_amd.engine_e import esrgan_discriminator_engine
    x, state = EO.d_inputs(2)
    d = EO.build_discriminator()
    assert all(torch.equal(v, state[k]) for k, v in d.state_dict().items())
    d.compute_dtype = MODES[mode]
    d.cuda().train()
    S = EO.F16_LOSS_SCALE if mode == "f16" else 1.0

    def one_pass():
        d.zero_grad(set_to_none=True)
        xg = x.cuda().requires_grad_(True)
        logits = d(xg)
        (F.binary_cross_entropy_with_logits(logits, torch.ones_like(logits)) * S).backward()
        torch.cuda.synchronize()
        out = {"logits": logits.detach().cpu(), "dx": xg.grad.cpu() / S}
        for k, p in d.named_parameters():
            out["grad." + k] = None if p.grad is None else p.grad.detach().cpu() / S
        out["tracked"] = [int(d.features[fi + 1].num_batches_tracked) for fi in EO.O.ESRGAN_D_CONVS[1:]]
        return out
    got = one_pass()
    sp = esrgan_discriminator_engine(d)._last
    nchw = lambda t: t.detach().float().permute(0, 3, 1, 2).cpu()             # noqa: E731
    for i in range(10):
        got["act.a%d" % i] = nchw(sp.a[i])
    got["act.f1"] = sp.f1.detach().float().cpu()[:, 0, 0, :100]
    for i in range(1, 10):
        # csrc/norm.hip, batchnorm_fwd_impl: ``save`` is [block][mean | invstd | scale | shift], channel blocks of <= 256
        c = sp.a[i].shape[-1]
        blocks = sp.save[i].detach().cpu().view(-1, 4, min(c, 256))
        got["bn.mean.%d" % i], got["bn.rstd.%d" % i] = blocks[:, 0].reshape(c), blocks[:, 1].reshape(c)
    for k, v in d.state_dict().items():
        if "running" in k:
            got["state." + k] = v.detach().cpu().clone()
    again = one_pass()
    for p in d.parameters():
        p.requires_grad = False
    frozen = one_pass()
    # the predicate the kernels apply to the STORED activation -- csrc/norm.hip, bn_partial_kernel / chan_affine_kernel:
    #     dv[q] *= av[q] > 0.f ? 1.f : act_slope;          va[q] *= vb[q] > 0.f ? 1.f : act_slope;
    # csrc/conv_igemm.hip, the mask path of the epilogue:  v *= (Elem<T>::to_f(mg[...]) > 0.f) ? 1.f : a.mask_slope;
    signs = [got["act." + k] > 0 for k in EO.ACTS]
    tags = ("f64", "f32") + ((mode,) if mode != "f32" else ())
    runs, probes = {}, {}
    for tag in tags:
        probes[tag] = {}
        runs[tag] = EO.discriminator(x, state, loss=EO.bce_ones, signs=signs, probe=probes[tag], **EO.run_kw(tag))
    return dict(got=got, again=again, frozen=frozen, signs=signs, runs=runs, probes=probes)


@pytest.mark.parametrize("mode", list(MODES))
def test_discriminator_matches_oracle(mode):
    """The sharp check of the BatchNorm discriminator (engine_e.py): one training forward and one loss-scaled backward of BCE against
    ones at N = 2 (x[:2] of the fixture), parameters and x requiring gradients, against tests/esrgan_d_oracle.discriminator in relative
    L2 under the rule -- f32: 8 G; f16 / bf16: max(2 E, 8 G), G the oracle's float32-vs-float64 gap, E its gap with that type's rounding
    points -- with the signs the engine's own plan stored (``a > 0`` on sp.a[0..9] and sp.f1) replayed in the DERIVATIVES of all oracle
    runs.  Compared: the logits, the eleven stored activations, the nine saved batch means and rstd (sp.save), the running statistics
    after the pass, dx and all 33 gradients as whole tensors.  tests/test_esrgan_d_host.py holds E to <= 1e-2 / 5e-2, so no 16-bit bound
    here exceeds 2e-2 / 1e-1 (measured: <= 5.6e-3 / 4.6e-2), and shows that the bound sees a LeakyReLU' slope of 0.25 or a constant
    rstd in one stage.  A sign may differ from the float64 run's only where the reference cannot decide it: no unit farther from zero
    than 8 x the largest deviation, at that layer, of the oracle at the mode's precision, and in the 16-bit modes a flipped share under
    flip_cap of the emulated oracle's own.  The two logits and classifier.2.bias's one gradient have floors (SCALAR_FLOOR's note).
    MI355X (profiles/esrgan_d_oracle_fp64.txt has every row, DESIGN.md 4i the table): f32 every tensor at 0.12 .. 0.98 of 8 G
    (bn.rstd.1 at 0.98 -- the statistics kernel's fp32 E[y^2] - mean^2 --, the other statistics <= 0.37, activations <= 0.39, dx 0.32,
    gradients <= 0.49); f16 0.14 .. 0.58 of max(2 E, 8 G) (an error equal to E is 0.5; dx 0.49, gradients 0.41 .. 0.58), bounds
    <= 5.0e-3; bf16 0.43 .. 0.54, bounds <= 4.3e-2.  Flipped LeakyReLU units: shares 4.0e-7 / 2.28e-4 / 1.87e-3 of 5.0 million (the oracle's own at
    that precision 0 / 2.28e-4 / 1.88e-3), the farthest at 0.21 / 0.66 / 0.66 of the oracle's largest deviation (8 allowed).  The logits against
    W2 f1 + b2 of the stored f1: 1.5e-8 .. 1.8e-8 of sum |w f1|; against the float64 oracle 1.8e-5 / 7.9e-3 / 3.2e-2 (0.79 / 1.40 /
    0.69 of the un-floored rule)."""
    r = _d_pass(mode)
    got, runs = r["got"], r["runs"]
    keys = [k for k in runs["f64"] if k != "loss" and not k.endswith("num_batches_tracked") and not k.startswith("bn.var.")]
    assert len(keys) == 1 + 11 + 18 + 18 + 1 + 33 and all(got[k] is not None and got[k].dtype == torch.float32 for k in keys)
    # FLOORS (see SCALAR_FLOOR's note).  u: the unit roundoff of the stored type.
    # logits = W2 f1 + b2 with W2 stored rounded: |d logits|_2 <= |W2|_2 (|d f1|_F + u |f1|_F), and the rule bounds |d f1|_F / |f1|_F;
    # classifier.2.bias's gradient g = sum_n (sigmoid(x_n) - 1) / N, each term stored rounded in sp.dl: sigmoid' <= 1/4, so
    # |d g| <= |d x|_1 / (4 N) + u |g| <= |d x|_2 / (4 sqrt(N)) + u |g|.
    # (|W2| |f1| / |logits| is 38 here -- the 100 terms cancel --, so the logits' floor is 38 x f1's bound: 5.5e-4 / 1.6e-1 / 1.6, on
    # its own no bound in bf16.  What pins the logits is f1 under the rule and the dot-product check below.)
    ref, u = runs["f64"], 0.0 if mode == "f32" else float(torch.finfo(MODES[mode]).eps) / 2
    W2, n = EO.d_inputs(2)[1]["classifier.2.weight"].double().norm(), ref["logits"].numel()
    floors = {"logits": lambda b: W2 * ref["act.f1"].norm() * (b["act.f1"] + u) / ref["logits"].norm(),
              "grad.classifier.2.bias": lambda b: b["logits"] * ref["logits"].norm() / (4 * n ** 0.5) / ref["grad.classifier.2.bias"].abs().sum() + u}
    bad = _rule("ESRGAN D", mode, got, runs, keys, floors)
    # ... and the two logits are pinned more sharply than the rule could: they are W2 f1 + b2 of the STORED f1 and the stored (rounded)
    # W2 in float64, within the roundoff of an fp32 dot product of 100 terms in any order (a product of two 16-bit values is exact in
    # fp32; f32: one rounding each): at most 102 roundings of 2^-24 relative to sum |w_i f1_i| + |b2|
    st = EO.d_inputs(2)[1]
    w2 = st["classifier.2.weight"].to(MODES[mode]).double()
    exact = got["act.f1"].double() @ w2.t() + st["classifier.2.bias"].double()
    scale = got["act.f1"].double().abs() @ w2.abs().t() + st["classifier.2.bias"].double().abs()
    e_dot = float(((got["logits"].double() - exact).abs() / scale).max())
    print("ESRGAN D     %-4s the logits against the float64 W2 f1 + b2 of the stored f1: %.3e of sum |w f1| (allowed 102 x 2^-24 = %.3e)" % (mode, e_dot, 102 * 2.0 ** -24))
    assert e_dot <= 102 * 2.0 ** -24
    rows = []
    for k, (mine, p64, pp) in enumerate(zip(r["signs"], r["probes"]["f64"]["pre"], r["probes"][mode]["pre"])):
        own = EO.positive(runs[mode]["act." + EO.ACTS[k]])
        rows.append(_flips("ESRGAN D", mode, EO.ACTS[k], mine, p64 > 0, own, p64.abs(), float((pp.double() - p64).abs().max())))
    _share_check("ESRGAN D", mode, "LeakyReLU", rows)
    assert not bad, bad
    assert got["tracked"] == [1] * 9


@pytest.mark.parametrize("mode", list(MODES))
def test_discriminator_passes_are_exact(mode):
    """A second pass gives the first one's bits (another plan of the engine's ring: other buffers, the same launches); a pass with the
    parameters frozen -- the fused trainer's generator phase: the same launch list without the weight-gradient items, the BatchNorm
    backward's parameter sums going to the scratch gradient -- gives the full pass's dx bit for bit; num_batches_tracked advances by one
    per training forward."""
    r = _d_pass(mode)
    got, again, frozen = r["got"], r["again"], r["frozen"]
    for k in again:
        if k != "tracked":
            assert torch.equal(got[k], again[k]), "two passes differ in " + k
    assert torch.equal(frozen["logits"], got["logits"]) and torch.equal(frozen["dx"], got["dx"]), "the frozen pass's dx differs"
    assert all(frozen[k] is None for k in frozen if k.startswith("grad."))
    assert got["tracked"] == [1] * 9 and again["tracked"] == [2] * 9 and frozen["tracked"] == [3] * 9


UPSTREAM = 2.5


@pytest.mark.parametrize("mode", list(MODES))
def test_content_loss_gradient_matches_oracle(mode):
    """The sharp check of the differentiable VGG content loss (engine_v.py, ContentLossGradEngine): ContentLoss("features.34") at
    2 x 3 x 48 x 32, seeded BEFORE the module is constructed, upstream factor 2.5 and, in f16, the loss scale 65536 through ``dloss``.
    The loss value and d/dSR against tests/esrgan_d_oracle.content_loss under the same rule, with the three kinds of discrete state
    taken from the engine's plan (sp.keep, sp.feat) and replayed in all oracle runs: the ReLU masks of the SR half (``> 0`` on the
    stored outputs, the conv epilogue's mask predicate), the pool routing derived from the stored pre-pool maps by
    maxpool2_relu_bwd_kernel's rule (first maximum in row-major order), the L1 sign of the stored tap halves as l1_grad_views_kernel
    computes it.  Each kind has its own flipped-state condition: no unit farther from its switch (the pre-activation from zero; the
    window's largest value from the second largest; the tap difference from zero) than 8 x the oracle's own largest deviation there
    (twice that for a routing: two values move), and in the 16-bit modes a share under flip_cap.  A second pass gives the same bits.
    MI355X (profiles/esrgan_d_oracle_fp64.txt): d/dSR at 0.47 / 0.50 / 0.50 of the bound (f32 / f16 / bf16; bounds 4.5e-6 /
    2.2e-3 / 1.7e-2, against the hand-set 1e-2 / 1.5e-1 / 4e-1 of the test above), the two halves of the tap map at 0.46 .. 0.51; the loss
    against the float64 mean of the stored halves 6.9e-8 .. 9.5e-8, against the oracle 7.8e-7 / 1.9e-4 / 3.3e-3.  Flipped shares -- ReLU
    1.1e-6 / 1.55e-4 / 1.17e-3 (the oracle's own 0 / 1.55e-4 / 1.20e-3), pool routing 0 / 4.4e-4 / 4.0e-3 (0 / 4.8e-4 / 3.8e-3), L1 sign 0 /
    3.3e-3 / 2.7e-2 (0 / 2.9e-3 / 2.5e-2) --, the farthest flipped unit at <= 0.70 of the oracle's largest deviation (8 allowed)."""
    from sr_gan_fd_amd.engine import _ENGINES
    sr, gt, P = EO.content_inputs()
    cl = EO.build_content_loss()
    assert all(torch.equal(v, P["features." + k]) for k, v in cl.features.state_dict().items())
    cl.compute_dtype = MODES[mode]
    cl.cuda()
    S = EO.F16_LOSS_SCALE if mode == "f16" else 1.0

    def one_pass():
        s = sr.cuda().requires_grad_(True)
        loss = cl(s, gt.cuda())
        (UPSTREAM * S * loss).backward()
        torch.cuda.synchronize()
        return {"loss": loss.detach().cpu(), "dsr": s.grad.cpu() / S}
    got = one_pass()
    sp = _ENGINES[cl]._last
    N = sr.shape[0]
    half = lambda t: t[:N].detach().float().permute(0, 3, 1, 2).cpu()         # noqa: E731
    chain = EO.vgg_chain()
    # sp.keep[1 + idx] is what features[idx] left: a conv's (+ ReLU's) output, the same map again for the ReLU module, the pooled map
    relu_maps = [half(sp.keep[1 + idx]) for kind, idx, relu in chain if kind == "conv" and relu]
    pool_maps = [half(sp.keep[idx]) for kind, idx, _ in chain if kind == "pool"]
    feat_sr, feat_gt = half(sp.feat), sp.feat[N:].detach().float().permute(0, 3, 1, 2).cpu()
    states = {"relu": [EO.positive(t) for t in relu_maps], "route": [EO.pool_route(t) for t in pool_maps], "sign": EO.l1_sign(feat_sr, feat_gt)}
    again = one_pass()
    assert torch.equal(got["loss"], again["loss"]) and torch.equal(got["dsr"], again["dsr"]), "two passes differ"
    tags = ("f64", "f32") + ((mode,) if mode != "f32" else ())
    runs, probes = {}, {}
    for tag in tags:
        probes[tag] = {}
        runs[tag] = EO.content_loss(sr, gt, P, upstream=UPSTREAM, states=states, probe=probes[tag], **EO.run_kw(tag))
    got["feat_sr"], got["feat_gt"] = feat_sr, feat_gt
    # the loss is ONE number (see SCALAR_FLOOR's note; measured against the un-floored rule: f32 1.06, f16 1.30, bf16 0.66 of it).  It is
    # pinned in two sharper ways instead: the two halves of the stored tap map it is computed from are held to the rule as tensors, and it
    # equals the float64 mean |sr_f - gt_f| of the STORED halves within the roundoff of its fp32 sum of non-negative terms
    # (csrc/loss.hip, l1_views_partial_kernel's vector form + finish_kernel<FinAxpy> over min(ceil(n / 256), 1024) blocks: the difference -- exact for
    # 16-bit values, one rounding in f32 --, a thread's serial chain over its vectors of at most 8 elements, at most 10 additions of
    # block_reduce_sum, the finish kernel's chain over the blocks' partials and its block_reduce_sum, the rounding of 1 / n and the
    # scaling: each one rounding of at most 2^-24).  Its floor under the rule is what the rule's bounds on the two halves allow:
    # |d loss| <= mean |d sr_f| + mean |d gt_f| <= rms(d sr_f) + rms(d gt_f), and rms(d f) <= bound * rms(f)
    n = feat_sr.numel()
    blocks = min(-(-n // 256), 1024)
    exact = float((feat_sr.double() - feat_gt.double()).abs().mean())
    roundings = 1 + 8 * -(-n // (8 * 256 * blocks)) + 10 + -(-blocks // 256) + 10 + 2
    e_sum = abs(float(got["loss"]) - exact) / exact
    print("content loss %-4s the loss against the float64 mean of the stored halves: %.3e (allowed %d x 2^-24 = %.3e)" % (mode, e_sum, roundings, roundings * 2.0 ** -24))
    assert e_sum <= roundings * 2.0 ** -24
    ref = runs["f64"]
    rms = lambda t: float(t.double().pow(2).mean().sqrt())                    # noqa: E731
    floors = {"loss": lambda b: (b["feat_sr"] * rms(ref["feat_sr"]) + b["feat_gt"] * rms(ref["feat_gt"])) / float(ref["loss"])}
    bad = _rule("content loss", mode, got, runs, ["feat_sr", "feat_gt", "loss", "dsr"], floors)
    p64, pp = probes["f64"], probes[mode]
    dev = lambda a, b: float((a.double() - b).abs().max())                    # noqa: E731
    rows = [_flips("content loss", mode, "relu %d" % k, states["relu"][k], p64["pre"][k] > 0, EO.positive(pp["maps"][k]), p64["pre"][k].abs(),
                   dev(pp["pre"][k], p64["pre"][k])) for k in range(len(relu_maps))]
    _share_check("content loss", mode, "ReLU", rows)
    rows = []
    for k in range(len(pool_maps)):
        w64 = EO.windows(p64["pre_pool"][k]).sort(-1, descending=True).values
        live = w64[..., 0] > 0                                                # (a window without a positive value passes no gradient)
        mine, r64, own = states["route"][k][live], EO.pool_route(p64["pre_pool"][k])[live], EO.pool_route(pp["pre_pool"][k])[live]
        rows.append(_flips("content loss", mode, "pool %d" % k, mine, r64, own, (w64[..., 0] - w64[..., 1])[live], 2 * dev(pp["pre_pool"][k], p64["pre_pool"][k])))
    _share_check("content loss", mode, "pool routing", rows)
    d64, dp = p64["maps"][-1] - p64["feat_gt"], pp["maps"][-1].double() - pp["feat_gt"].double()
    rows = [_flips("content loss", mode, "L1 sign", states["sign"], torch.sign(d64), torch.sign(dp), d64.abs(), dev(dp, d64))]
    _share_check("content loss", mode, "L1 sign", rows)
    assert not bad, bad
