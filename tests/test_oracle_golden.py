"""Pin the CPU oracle (oracle/srgan_oracle.py) to golden vectors captured from the reference.

Runs on CPU (`-m "not gpu"`).  Weights are rebuilt from the seed with this repository's parameter
containers (sr_gan_fd_amd.model); the per-tensor checksums stored in the fixtures prove the rebuild
is bit-identical to the reference's constructors before any output is compared.
"""
import numpy as np
import pytest
import torch

from tests.util import checksum, load_golden, pinned_vgg, scaled_init, table, sd_to_params

TOL = 2e-5  # fp32 CPU vs fp32 CPU: only op-ordering noise


def _close(a, b, tol=TOL, what=""):
    a = torch.as_tensor(np.asarray(a)).double()
    b = torch.as_tensor(np.asarray(b)).double()
    scale = b.abs().max().item() + 1e-30
    err = (a - b).abs().max().item() / scale
    assert err < tol, f"{what}: rel err {err:.3e}"


def _check_table(tab, named, tol=1e-9, what=""):
    for k, want in tab.items():
        got = checksum(named[k])
        assert np.allclose(got, want, rtol=tol, atol=tol * (abs(want[1]) + 1e-30)), f"{what} checksum {k}: {got} vs {want}"


def test_blocks(golden_dir):
    from oracle import srgan_oracle as O
    from sr_gan_fd_amd import model as M
    g = load_golden(golden_dir, "blocks.npz")
    for kind, ctor in (("rdb", M._ResidualDenseBlock), ("rrdb", M._ResidualResidualDenseBlock)):
        torch.manual_seed(0)
        blk = ctor(64, 32)
        _check_table(table(g, f"{kind}_wsum"), blk.state_dict(), what=kind)
        P = sd_to_params(blk.state_dict(), grad=True)
        x = torch.tensor(g[f"{kind}_x"], requires_grad=True)
        y = O.rdb_forward(x, P, "") if kind == "rdb" else O.rrdb_forward(x, P, "")
        _close(y.detach(), g[f"{kind}_y"], what=f"{kind} y")
        (y * torch.tensor(g[f"{kind}_r"])).sum().backward()
        _close(x.grad, g[f"{kind}_dx"], what=f"{kind} dx")
        for k, want in table(g, f"{kind}_gsum").items():
            got = checksum(P[k].grad)
            assert np.allclose(got, want, rtol=1e-4, atol=1e-4 * abs(want[1])), f"{kind} grad checksum {k}"


@pytest.mark.parametrize("name,fac,kw,s,scale", [
    ("bsrgan_x4_r2_s3", "bsrgan_x4", dict(num_rrdb=2), 4, 3.0),
    ("bsrgan_x2_r2_s3", "bsrgan_x2", dict(num_rrdb=2), 2, 3.0),
    ("bsrgan_x4_r2_s5", "bsrgan_x4", dict(num_rrdb=2), 4, 5.0),
    ("rrdbnet_x4_r23_s3", "rrdbnet_x4", dict(num_blocks=23), 4, 3.0),
    ("bsrgan_x4_r23_s3_odd", "bsrgan_x4", dict(num_rrdb=23), 4, 3.0),
])
def test_generator(golden_dir, name, fac, kw, s, scale):
    from oracle import srgan_oracle as O
    from sr_gan_fd_amd import model as M
    g = load_golden(golden_dir, "generator.npz")
    torch.manual_seed(0)
    net = getattr(M, fac)(in_channels=3, out_channels=3, channels=64, growth_channels=32, **kw)
    scaled_init(net, scale, 0.5)
    _check_table(table(g, f"{name}/wsum"), net.state_dict(), what=name)
    P = sd_to_params(net.state_dict(), grad=True)
    sr = O.rrdbnet_forward(torch.tensor(g[f"{name}/x"]), P, s)
    _close(sr.detach(), g[f"{name}/sr"], what="sr")
    loss = O.l1_mean(sr, torch.tensor(g[f"{name}/gt"]))
    assert abs(loss.item() - float(g[f"{name}/loss"])) < 1e-6
    loss.backward()
    for k in ("conv1.weight", "conv4.weight", "conv4.bias", "trunk.0.rdb1.conv1.bias", "trunk.1.rdb3.conv5.bias", "conv2.bias"):
        _close(P[k].grad, g[f"{name}/grad/{k}"], tol=2e-4, what=f"grad {k}")
    for k, want in table(g, f"{name}/gsum").items():
        got = checksum(P[k].grad)
        assert np.allclose(got, want, rtol=2e-3, atol=2e-4 * abs(want[1]) + 1e-12), f"{name} grad checksum {k}: {got} {want}"


@pytest.mark.parametrize("name,s", [("x2_r2_s3", 2), ("x1_r2_s3", 1), ("x2_r2_s3_odd", 2)])
def test_realesrgan_rrdbnet_below_x4(golden_dir, name, s):
    """Real_ESRGAN/model.py:190-204,248: PixelUnshuffle(4 / s) in front of conv1, both upsampling stages (fixture from the reference class)"""
    from oracle import srgan_oracle as O
    from sr_gan_fd_amd import model as M
    g = load_golden(golden_dir, "realesrgan_rrdbnet.npz")
    torch.manual_seed(0)
    net = M.RRDBNet(in_channels=3, out_channels=3, channels=64, growth_channels=32, num_rrdb=2, upscale_factor=s)
    scaled_init(net, 3.0, 0.5)
    _check_table(table(g, f"{name}/wsum"), net.state_dict(), what=name)
    P = sd_to_params(net.state_dict(), grad=True)
    sr = O.rrdbnet_forward(torch.tensor(g[f"{name}/x"]), P, 4, unshuffle=4 // s)
    _close(sr.detach(), g[f"{name}/sr"], what="sr")
    loss = O.l1_mean(sr, torch.tensor(g[f"{name}/gt"]))
    assert abs(loss.item() - float(g[f"{name}/loss"])) < 1e-6
    loss.backward()
    for k in ("conv1.weight", "conv1.bias", "conv4.weight", "trunk.0.rdb1.conv1.bias", "trunk.1.rdb3.conv5.bias", "conv2.bias"):
        _close(P[k].grad, g[f"{name}/grad/{k}"], tol=2e-4, what=f"grad {k}")


@pytest.mark.parametrize("name,s", [("x2_r2_s3", 2), ("x1_r2_s3", 1), ("x2_r2_s3_odd", 2)])
def test_realesrgan_below_x4_oracle_steps_take_unshuffle(golden_dir, name, s):
    """The oracle's step functions forward ``unshuffle`` to rrdbnet_forward (the GPU tests of the fused trainers below x4 rest on it):
    g_only_step from the fixture's weights returns the reference class's loss and SR, and each GAN step function's SR has the GT's
    shape (a step that dropped the keyword would produce a 4 / s times larger SR, or fail on conv1's 12 / 48 input channels)."""
    from oracle import srgan_oracle as O
    from sr_gan_fd_amd import model as M
    g = load_golden(golden_dir, "realesrgan_rrdbnet.npz")
    torch.manual_seed(0)
    net = M.RRDBNet(in_channels=3, out_channels=3, channels=64, growth_channels=32, num_rrdb=2, upscale_factor=s)
    scaled_init(net, 3.0, 0.5)
    _check_table(table(g, f"{name}/wsum"), net.state_dict(), what=name)
    G = sd_to_params(net.state_dict())
    x, gt = torch.tensor(g[f"{name}/x"]), torch.tensor(g[f"{name}/gt"])
    loss, sr = O.g_only_step(G, O.AdamState(G, O.g_param_names(G)), x, gt, upscale=4, lr=1e-4, betas=(0.9, 0.99), eps=1e-4,
                             unshuffle=4 // s)
    _close(sr, g[f"{name}/sr"], what="sr")
    assert abs(loss - float(g[f"{name}/loss"])) < 1e-6
    assert not torch.equal(G["conv1.weight"], net.conv1.weight)          # and the step did update the weights
    # the GAN step functions: a U-Net discriminator needs sides that are multiples of 8 (the odd fixture has none)
    if name.endswith("odd"):
        return
    torch.manual_seed(1)
    D0 = sd_to_params(M.discriminator_unet(in_channels=3, out_channels=1, channels=64).state_dict(), d=True)
    for step in ("gan_step", "realesrgan_gan_step"):
        G, D = sd_to_params(net.state_dict()), {k: v.clone() for k, v in D0.items()}
        opts = (O.AdamState(G, O.g_param_names(G)), O.AdamState(D, O.d_param_names(D)))
        if step == "gan_step":
            out = O.gan_step(G, D, *opts, x, gt, upscale=4, g_lr=1e-4, d_lr=1e-4, betas=(0.9, 0.99), eps=1e-4, pixel_weight=1.0,
                             content_weight=1.0, adversarial_weight=0.1, unshuffle=4 // s)
        else:
            out = O.realesrgan_gan_step(G, D, *opts, x, gt, gt, unshuffle=4 // s)
        _close(out["sr"], g[f"{name}/sr"], what=f"{step} sr")
        assert abs(out["pixel_loss"] - float(g[f"{name}/loss"])) < 1e-6, step


def test_discriminator(golden_dir):
    from oracle import srgan_oracle as O
    from sr_gan_fd_amd import model as M
    g = load_golden(golden_dir, "discriminator.npz")
    torch.manual_seed(0)
    d = M.discriminator_unet(in_channels=3, out_channels=1, channels=64)
    _check_table(table(g, "wsum0"), d.state_dict(), what="D")
    P = sd_to_params(d.state_dict(), grad=True, d=True)
    x = torch.tensor(g["x"])
    for it in range(3):
        logits = O.discriminator_unet_forward(x, P, training=True)
        _close(logits.detach(), g[f"train{it}_logits"], what=f"logits {it}")
        for layer in ("down_block1", "up_block1", "conv3"):
            _close(P[f"{layer}.0.weight_u"], g[f"train{it}_{layer}_u"], what="u")
            _close(P[f"{layer}.0.weight_v"], g[f"train{it}_{layer}_v"], what="v")
    loss = O.bce_with_logits_mean(logits, 1.0)
    assert abs(loss.item() - float(g["bce_ones"])) < 1e-6
    loss.backward()
    for k in ("conv1.weight", "conv4.weight", "conv4.bias", "conv3.0.weight_orig"):
        _close(P[k].grad, g[f"grad/{k}"], tol=2e-4, what=f"grad {k}")
    for k, want in table(g, "gsum").items():
        got = checksum(P[k].grad)
        assert np.allclose(got, want, rtol=2e-3, atol=2e-4 * abs(want[1]) + 1e-12), f"D grad checksum {k}"
    with torch.no_grad():
        _close(O.discriminator_unet_forward(x, P, training=False), g["eval_logits"], what="eval logits")
    xin = x.clone().requires_grad_(True)
    lg = O.discriminator_unet_forward(xin, P, training=True)
    _close(lg.detach(), g["train3_logits"], what="logits 3")
    O.bce_with_logits_mean(lg, 1.0).backward()
    _close(xin.grad, g["train3_dx"], tol=2e-4, what="dx")


def test_gan_steps(golden_dir):
    """two iterations of train_bsrgan.py:387-483 (content loss = 0: no VGG weights in the reference tree)"""
    from oracle import srgan_oracle as O
    from sr_gan_fd_amd import model as M
    g = load_golden(golden_dir, "gan_steps.npz")
    torch.manual_seed(0)
    d = M.discriminator_unet(in_channels=3, out_channels=1, channels=64)
    gen = M.bsrgan_x4(in_channels=3, out_channels=3, channels=64, growth_channels=32, num_rrdb=2)
    scaled_init(gen, 3.0, 0.5)
    _check_table(table(g, "wsum_g0"), gen.state_dict(), what="G0")
    _check_table(table(g, "wsum_d0"), d.state_dict(), what="D0")
    G = sd_to_params(gen.state_dict())
    D = sd_to_params(d.state_dict(), d=True)
    g_opt = O.AdamState(G, O.g_param_names(G))
    d_opt = O.AdamState(D, O.d_param_names(D))
    ema, n_avg = {}, 0
    for it in range(2):
        out = O.gan_step(G, D, g_opt, d_opt, torch.tensor(g[f"it{it}_lr"]), torch.tensor(g[f"it{it}_gt"]), upscale=4,
                         g_lr=8e-5, d_lr=2e-4, betas=(0.9, 0.999), eps=1e-4, pixel_weight=20.0, content_weight=1.0,
                         adversarial_weight=0.5)
        n_avg = O.ema_update(ema, {k: G[k] for k in O.g_param_names(G)}, n_avg, 0.999)
        want = g[f"it{it}_scalars"]
        got = [out["d_loss"], out["pixel_loss"], out["content_loss"], out["adversarial_loss"],
               out["d_gt_probability"], out["d_sr_probability"]]
        assert np.allclose(got, want, rtol=2e-5, atol=1e-6), f"it{it}: {got} vs {want}"
        _close(G["conv4.bias"], g[f"it{it}_g_conv4_bias"], tol=1e-5, what="G conv4.bias")
        _close(D["conv4.weight"], g[f"it{it}_d_probe"], tol=1e-5, what="D conv4.weight")
        for k, want_c in table(g, f"it{it}_wsum_g").items():
            assert np.allclose(checksum(G[k]), want_c, rtol=1e-4, atol=1e-5 * abs(want_c[1])), f"G {k}"
        for k, want_c in table(g, f"it{it}_wsum_d").items():
            assert np.allclose(checksum(D[k]), want_c, rtol=1e-4, atol=1e-5 * abs(want_c[1])), f"D {k}"
        for k, want_c in table(g, f"it{it}_wsum_ema").items():
            if k == "n_averaged":
                continue
            assert np.allclose(checksum(ema[k[len("module."):]]), want_c, rtol=1e-4, atol=1e-5 * abs(want_c[1])), f"EMA {k}"


def test_realesrgan_gan_steps(golden_dir):
    """two iterations of Real_ESRGAN/train_realesrgan.py:407-476 (generator first, USM-sharpened GT for the pixel loss) around
    Real_ESRGAN/model.py's own RRDBNet / DiscriminatorUNet"""
    from oracle import srgan_oracle as O
    from sr_gan_fd_amd import model as M
    g = load_golden(golden_dir, "realesrgan_gan_steps.npz")
    torch.manual_seed(0)
    d = M.discriminator_unet(in_channels=3, out_channels=1, channels=64)
    gen = M.rrdbnet_x4(in_channels=3, out_channels=3, channels=64, growth_channels=32, num_rrdb=2)
    scaled_init(gen, 3.0, 0.5)
    _check_table(table(g, "wsum_g0"), gen.state_dict(), what="G0")
    _check_table(table(g, "wsum_d0"), d.state_dict(), what="D0")
    G = sd_to_params(gen.state_dict())
    D = sd_to_params(d.state_dict(), d=True)
    g_opt, d_opt = O.AdamState(G, O.g_param_names(G)), O.AdamState(D, O.d_param_names(D))
    ema, n_avg = {}, 0
    for it in range(2):
        out = O.realesrgan_gan_step(G, D, g_opt, d_opt, torch.tensor(g[f"it{it}_lr"]), torch.tensor(g[f"it{it}_gt"]), torch.tensor(g[f"it{it}_gt_usm"]))
        n_avg = O.ema_update(ema, {k: G[k] for k in O.g_param_names(G)}, n_avg, 0.999)
        got = [out["d_loss"], out["pixel_loss"], out["content_loss"], out["adversarial_loss"], out["d_gt_probability"], out["d_sr_probability"]]
        assert np.allclose(got, g[f"it{it}_scalars"], rtol=2e-5, atol=1e-6), f"it{it}: {got} vs {g[f'it{it}_scalars']}"
        _close(out["sr"], g[f"it{it}_sr"], what="sr")
        _close(G["conv4.bias"], g[f"it{it}_g_conv4_bias"], tol=1e-5, what="G conv4.bias")
        _close(D["conv4.weight"], g[f"it{it}_d_probe"], tol=1e-5, what="D conv4.weight")
        for P, key in ((G, f"it{it}_wsum_g"), (D, f"it{it}_wsum_d")):
            for k, want_c in table(g, key).items():
                assert np.allclose(checksum(P[k]), want_c, rtol=1e-4, atol=1e-5 * abs(want_c[1])), f"{key} {k}"
        for k, want_c in table(g, f"it{it}_wsum_ema").items():
            if k != "n_averaged":
                assert np.allclose(checksum(ema[k[len("module."):]]), want_c, rtol=1e-4, atol=1e-5 * abs(want_c[1])), f"EMA {k}"


@pytest.mark.parametrize("name,fac,kw,lr,eps", [
    ("esrgan_small", "rrdbnet_x4", dict(num_blocks=2), 2e-4, 1e-8),
    ("bsrnet_small", "bsrgan_x4", dict(num_rrdb=2), 1e-4, 1e-4),
])
def test_g_only_steps(golden_dir, name, fac, kw, lr, eps):
    from oracle import srgan_oracle as O
    from sr_gan_fd_amd import model as M
    g = load_golden(golden_dir, "g_only_steps.npz")
    torch.manual_seed(0)
    net = getattr(M, fac)(in_channels=3, out_channels=3, channels=64, growth_channels=32, **kw)
    scaled_init(net, 3.0, 0.5)
    G = sd_to_params(net.state_dict())
    opt = O.AdamState(G, O.g_param_names(G))
    for it in range(2):
        loss, sr = O.g_only_step(G, opt, torch.tensor(g[f"{name}/it{it}_lr"]), torch.tensor(g[f"{name}/it{it}_gt"]),
                                 upscale=4, lr=lr, betas=(0.9, 0.99), eps=eps)
        assert abs(loss - g[f"{name}/losses"][it]) < 2e-6
        _close(sr, g[f"{name}/it{it}_sr"], what="sr")
        for k, want_c in table(g, f"{name}/it{it}_wsum").items():
            assert np.allclose(checksum(G[k]), want_c, rtol=1e-4, atol=1e-5 * abs(want_c[1])), f"{name} {k}"
    _close(G["conv4.bias"], g[f"{name}/conv4_bias"], tol=1e-5, what="conv4.bias")


def test_psnr_definition():
    """_psnr_torch (image_quality_assessment.py:361-395): identical images -> 10*log10(255^2/1e-8)"""
    from oracle import srgan_oracle as O
    a = torch.rand(2, 3, 8, 8)
    assert torch.allclose(O.psnr_y(a, a), torch.full((2,), 10 * np.log10(255.0 ** 2 / 1e-8), dtype=torch.float64))
    b = (a + 0.1).clamp(0, 1)
    y = lambda t: ((t * torch.tensor([65.481, 128.553, 24.966]).view(1, 3, 1, 1)).sum(1, keepdim=True) + 16.0) / 255.0
    mse = ((y(a).double() * 255 - y(b).double() * 255) ** 2 + 1e-8).mean(dim=[1, 2, 3])
    assert torch.allclose(O.psnr_y(a, b), 10 * torch.log10(255.0 ** 2 / mse), rtol=1e-6)


def test_aesrgan_discriminator(golden_dir):
    """UNetDiscriminatorAesrgan (A-ESRGAN/model.py:279-345) oracle vs vectors captured from the reference"""
    from oracle import srgan_oracle as O
    from sr_gan_fd_amd import model as M
    g = load_golden(golden_dir, "aesrgan_discriminator.npz")
    torch.manual_seed(0)
    d = M.UNetDiscriminatorAesrgan(3)
    _check_table(table(g, "wsum0"), d.state_dict(), what="A-ESRGAN D")
    P = {k: v.detach().clone() for k, v in d.state_dict().items()}
    names = [k for k, _ in d.named_parameters()]
    for k in names:
        P[k].requires_grad_(True)
    x = torch.tensor(g["x"])
    for it in range(2):
        logits, (s1, s2, s3) = O.aesrgan_unet_forward(x, P, training=True, return_attention=True)
        _close(logits.detach(), g[f"train{it}_logits"], what=f"logits {it}")
        _close(s3.detach(), g[f"train{it}_attn3"], what="attention map 3")
        for k, want in table(g, f"train{it}_statesum").items():
            assert np.allclose(checksum(P[k]), want, rtol=1e-4, atol=1e-5 * abs(want[1]) + 1e-9), f"state {k}"
    loss = O.bce_with_logits_mean(logits, 1.0)
    assert abs(loss.item() - float(g["bce_ones"])) < 1e-6
    grads = dict(zip(names, torch.autograd.grad(loss, [P[k] for k in names])))
    for k in ("conv0.weight", "conv9.weight", "conv9.bias", "attn_1.W.1.weight", "attn_1.W.1.bias", "attn_3.psi.weight",
              "attn_2.theta.weight", "attn_3.phi.bias", "gating.weight_orig"):
        _close(grads[k], g[f"grad/{k}"], tol=5e-4, what=f"grad {k}")
    for k, want in table(g, "gsum").items():
        # a bias in front of BatchNorm has a mathematically zero gradient (pure rounding noise): absolute floor
        assert np.allclose(checksum(grads[k]), want, rtol=5e-3, atol=5e-4 * abs(want[1]) + 1e-6), f"grad checksum {k}"
    with torch.no_grad():
        _close(O.aesrgan_unet_forward(x, P, training=False), g["eval_logits"], what="eval logits")
    xin = x.clone().requires_grad_(True)
    lg = O.aesrgan_unet_forward(xin, P, training=True)
    _close(lg.detach(), g["train2_logits"], what="logits 2")
    dx, = torch.autograd.grad(O.bce_with_logits_mean(lg, 1.0), xin)
    _close(dx, g["train2_dx"], tol=5e-4, what="dx")


def test_aesrgan_gan_steps(golden_dir):
    """two iterations of A-ESRGAN/train_aesrgan.py:396-483: RRDBNet x4 + attention U-Net discriminator (config 5 pairing)"""
    from oracle import srgan_oracle as O
    from sr_gan_fd_amd import model as M
    g = load_golden(golden_dir, "aesrgan_gan_steps.npz")
    torch.manual_seed(0)
    d = M.uNetDiscriminatorAesrgan()
    gen = M.bsrgan_x4(in_channels=3, out_channels=3, channels=64, growth_channels=32, num_rrdb=2)
    scaled_init(gen, 3.0, 0.5)
    _check_table(table(g, "wsum_g0"), gen.state_dict(), what="G0")
    _check_table(table(g, "wsum_d0"), d.state_dict(), what="D0")
    G = sd_to_params(gen.state_dict())
    D = {k: v.detach().clone() for k, v in d.state_dict().items()}
    g_opt = O.AdamState(G, O.g_param_names(G))
    d_opt = O.AdamState(D, O.d_param_names(D))
    for it in range(2):
        out = O.gan_step(G, D, g_opt, d_opt, torch.tensor(g[f"it{it}_lr"]), torch.tensor(g[f"it{it}_gt"]), upscale=4,
                         g_lr=5e-5, d_lr=1e-5, betas=(0.9, 0.999), eps=1e-4, pixel_weight=10.0, content_weight=1.0,
                         adversarial_weight=0.1, d_forward=O.aesrgan_unet_forward)
        want = g[f"it{it}_scalars"]
        got = [out["d_loss"], out["pixel_loss"], out["content_loss"], out["adversarial_loss"],
               out["d_gt_probability"], out["d_sr_probability"]]
        assert np.allclose(got, want, rtol=2e-5, atol=1e-6), f"it{it}: {got} vs {want}"
        _close(G["conv4.bias"], g[f"it{it}_g_conv4_bias"], tol=1e-5, what="G conv4.bias")
        _close(D["conv9.weight"], g[f"it{it}_d_probe"], tol=1e-5, what="D conv9.weight")
        # Iteration 0 is exact to rounding.  Iteration 1 starts from parameters that differ from the reference's by
        # ~5e-5 in a few biases (cancelling 8192-term sums), which is enough to flip a LeakyReLU mask inside G: measured
        # against the reference run side by side here, upsampling1/trunk gradients then differ by 2-4e-3 while
        # upsampling2/conv4 agree to 1e-5.  The iteration-1 bound is sized for that.
        rt, at = (1e-4, 1e-5) if it == 0 else (1e-4, 2e-2)
        for k, want_c in table(g, f"it{it}_wsum_g").items():
            assert np.allclose(checksum(G[k]), want_c, rtol=rt, atol=at * abs(want_c[1])), f"G {k}"
        for k, want_c in table(g, f"it{it}_wsum_d").items():
            assert np.allclose(checksum(D[k]), want_c, rtol=rt, atol=at * abs(want_c[1])), f"D {k}"


def test_validation_side(golden_dir):
    """_psnr_torch, _ssim_torch and random_crop restatements vs vectors captured from the reference (cv2 stubbed: neither uses it)"""
    import random
    from oracle import srgan_oracle as O
    g = load_golden(golden_dir, "validation.npz")
    a, b = torch.tensor(g["psnr_a"]), torch.tensor(g["psnr_b"])
    assert np.allclose(O.psnr_y(a, b, 4, True).numpy(), g["psnr_y_cb4"], rtol=0, atol=1e-9)
    assert np.allclose(O.psnr_y(a, b, 4, False).numpy(), g["psnr_rgb_cb4"], rtol=0, atol=1e-9)
    assert np.allclose(O.psnr_y(a, b, 0, True).numpy(), g["psnr_y_cb0"], rtol=0, atol=1e-9)
    # SSIM (image_quality_assessment.py:420-494): the reference's own functions were driven with the documented OpenCV window
    assert np.allclose(O.gaussian_window(11, 1.5), g["ssim_window"], rtol=0, atol=1e-16)
    for cb, y, key in ((4, True, "ssim_y_cb4"), (4, False, "ssim_rgb_cb4"), (0, True, "ssim_y_cb0")):
        assert np.allclose(O.ssim(a, b, cb, y).numpy(), g[key], rtol=0, atol=1e-7), key
    assert np.allclose(O.ssim(a, torch.roll(b, 3, dims=3), 0, True).numpy(), g["ssim_y_rolled"], rtol=0, atol=1e-7)
    assert np.allclose(O.ssim(a, b, 2, False, np.full((7, 7), 1.0 / 49.0)).numpy(), g["ssim_box7_rgb_cb2"], rtol=0, atol=1e-7)
    assert np.allclose(O.ssim(a, a, 0, True).numpy(), 1.0, rtol=0, atol=1e-7)                       # identical images
    gt, lr = torch.tensor(g["crop_gt"]), torch.tensor(g["crop_lr"])
    for seed in (7, 11):
        random.seed(seed)
        pg, pl = O.random_crop(gt, lr, 32, 4)
        assert np.array_equal(pg.numpy(), g[f"crop{seed}_gt"]) and np.array_equal(pl.numpy(), g[f"crop{seed}_lr"])


PIPE_PARAMS = dict(first_blur_probability=1.0, resize_probability1=[0.2, 0.7, 0.1], resize_range1=[0.15, 1.5], gray_noise_probability1=0.4,
                   gaussian_noise_probability1=0.5, noise_range1=[1, 30], poisson_scale_range1=[0.05, 3], jpeg_range1=[30, 95],
                   second_blur_probability=0.8, resize_probability2=[0.3, 0.4, 0.3], resize_range2=[0.3, 1.2], gray_noise_probability2=0.4,
                   gaussian_noise_probability2=0.5, noise_range2=[1, 25], poisson_scale_range2=[0.05, 2.5], jpeg_range2=[30, 95])


def test_degradation_oracle(golden_dir):
    """Real_ESRGAN/imgproc.py restatements (filter2d_torch, USMSharp, DiffJPEG, the noise stages, degradation_process) vs
    outputs of the reference's own functions: same torch CPU ops and the same generator stream, so bit-exact."""
    import random
    from oracle import degradation_oracle as D
    g = load_golden(golden_dir, "degradation.npz")
    T = lambda k: torch.tensor(g[k])
    same = lambda a, k: np.array_equal(a.numpy(), g[k])
    img = T("image")
    assert same(D.filter2d(img, T("kernels21")), "filter2d_per_image") and same(D.filter2d(img, T("kernels21")[:1]), "filter2d_shared")
    assert same(D.filter2d(img, T("kernel7")), "filter2d_k7")
    assert same(D.usm_kernel(50, 0), "usm_kernel")
    assert same(D.usm_sharp(T("usm_image"), D.usm_kernel(), 0.5, 10), "usm_w05_t10") and same(D.usm_sharp(T("usm_image"), D.usm_kernel(), 1.5, 3), "usm_w15_t3")
    f = D.quality_to_factor(T("jpeg_quality"))
    assert same(f, "jpeg_factor") and same(D.diff_jpeg(img, f), "jpeg") and same(D.diff_jpeg(img, f, True), "jpeg_diff")
    assert same(D.diff_jpeg(img[:, :, :32, :48], torch.full((3,), 0.8)), "jpeg_scalar_q60")
    sigma, gray = torch.tensor([5.0, 20.0, 12.0]), torch.tensor([0.0, 1.0, 0.0])
    torch.manual_seed(123)
    assert same(D.add_gaussian_noise(img, sigma, True, False, gray), "gauss_gray")
    torch.manual_seed(124)
    assert same(D.add_gaussian_noise(img, sigma, True, True, torch.zeros(3)), "gauss_color_rounds")
    torch.manual_seed(125)
    assert same(D.random_add_gaussian_noise(img, [1, 30], 0.4), "gauss_random")
    torch.manual_seed(126)
    assert same(D.add_poisson_noise(T("poisson_image"), torch.tensor([0.5, 2.0, 1.0]), True, False, 0), "poisson_color")
    torch.manual_seed(127)
    assert same(D.random_add_poisson_noise(T("poisson_image"), [0.05, 3], 0.0), "poisson_random")
    for seed in g["pipe_seeds"]:
        seed = int(seed)
        random.seed(seed); np.random.seed(seed); torch.manual_seed(seed)
        _, _, lr = D.degradation_process(T("pipe_gt"), T("pipe_k1"), T("pipe_k2"), T("pipe_sinc"), 4, PIPE_PARAMS)
        assert same(lr, f"pipe_lr_seed{seed}"), seed
    for seed in (3, 8):                                            # random_crop_torch on [gt_usm, gt], lr
        random.seed(seed)
        (a, b), (c,) = D.random_crop_lists([T("aug_gt") * 0.5, T("aug_gt")], [T("aug_lr")], 32, 4)
        assert same(a, f"aug_crop{seed}_gt_usm") and same(b, f"aug_crop{seed}_gt") and same(c, f"aug_crop{seed}_lr")


def _esrgan_d():
    from sr_gan_fd_amd import model as M
    torch.manual_seed(0)
    d = M.discriminator()
    with torch.no_grad():
        for m in d.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.3, 0.3)
    return d


def test_esrgan_discriminator(golden_dir):
    """Discriminator (ESRGAN/model.py:88-141) oracle vs vectors captured from the reference"""
    from oracle import srgan_oracle as O
    g = load_golden(golden_dir, "esrgan_discriminator.npz")
    d = _esrgan_d()
    _check_table(table(g, "wsum0"), d.state_dict(), what="ESRGAN D")
    P = {k: v.detach().clone() for k, v in d.state_dict().items()}
    names = [k for k, _ in d.named_parameters()]
    for k in names:
        P[k].requires_grad_(True)
    x = torch.tensor(g["x"])
    for it in range(2):
        logits = O.esrgan_discriminator_forward(x, P, training=True)
        _close(logits.detach(), g[f"train{it}_logits"], what=f"logits {it}")
        for k, want in table(g, f"train{it}_statesum").items():
            assert np.allclose(checksum(P[k]), want, rtol=1e-4, atol=1e-5 * abs(want[1]) + 1e-9), f"state {k}"
    loss = O.bce_with_logits_mean(logits, 1.0)
    assert abs(loss.item() - float(g["bce_ones"])) < 1e-6
    grads = dict(zip(names, torch.autograd.grad(loss, [P[k] for k in names])))
    for key in g.files:
        if key.startswith("grad/"):
            _close(grads[key[5:]], g[key], tol=1e-3, what=key)
        elif key.startswith("gradrows/"):
            _close(grads[key[9:]][:2], g[key], tol=1e-3, what=key)
    with torch.no_grad():
        _close(O.esrgan_discriminator_forward(x, P, training=False), g["eval_logits"], what="eval logits")
    xin = x.clone().requires_grad_(True)
    lg = O.esrgan_discriminator_forward(xin, P, training=True)
    _close(lg.detach(), g["train2_logits"], what="logits 2")
    dx, = torch.autograd.grad(O.bce_with_logits_mean(lg, 1.0), xin)
    ref = torch.tensor(g["train2_dx"])
    assert ((dx - ref).norm() / ref.norm()).item() < 1e-3        # L2: single LeakyReLU mask ties move isolated patches (see A-ESRGAN note)


def test_esrgan_gan_steps(golden_dir):
    """two iterations of ESRGAN/train_esrgan.py:364-431 (relativistic-average GAN, BatchNorm discriminator)"""
    from oracle import srgan_oracle as O
    from sr_gan_fd_amd import model as M
    g = load_golden(golden_dir, "esrgan_gan_steps.npz")
    torch.manual_seed(0)
    d = M.discriminator()
    gen = M.rrdbnet_x4(in_channels=3, out_channels=3, channels=64, growth_channels=32, num_blocks=2)
    scaled_init(gen, 3.0, 0.5)
    _check_table(table(g, "wsum_g0"), gen.state_dict(), what="G0")
    _check_table(table(g, "wsum_d0"), d.state_dict(), what="D0")
    G = sd_to_params(gen.state_dict())
    D = {k: v.detach().clone() for k, v in d.state_dict().items()}
    g_opt = O.AdamState(G, O.g_param_names(G))
    d_opt = O.AdamState(D, [k for k in D if k.endswith((".weight", ".bias"))])
    for it in range(2):
        out = O.esrgan_gan_step(G, D, g_opt, d_opt, torch.tensor(g[f"it{it}_lr"]), torch.tensor(g[f"it{it}_gt"]))
        got = [out["d_loss"], out["pixel_loss"], out["adversarial_loss"], out["d_gt_probability"], out["d_sr_probability"]]
        want = g[f"it{it}_scalars"]
        assert np.allclose(got, want, rtol=1e-4, atol=1e-6), f"it{it}: {got} vs {want}"
        _close(out["sr"][:, :, ::4, ::4], g[f"it{it}_sr"], tol=1e-4, what="sr")
        # esrgan_config's Adam eps is 1e-8: the first steps are lr * g / (|g| + 1e-8), i.e. lr * sign(g) even for gradient
        # entries that are rounding noise (near-cancelling bias sums), so a few entries per tensor legitimately land on
        # the other side; the bound allows ~3 % of a tensor's abs-sum.  Scalars and SR above are the tight checks.
        at = 5e-2
        bad = []
        for k, want_c in table(g, f"it{it}_wsum_g").items():
            if not np.allclose(checksum(G[k]), want_c, rtol=1e-4, atol=at * abs(want_c[1]) + 1e-9):
                bad.append((k, checksum(G[k]), want_c))
        assert not bad, bad[:3]
        for k, want_c in table(g, f"it{it}_wsum_d").items():
            if not k.endswith("num_batches_tracked"):
                assert np.allclose(checksum(D[k]), want_c, rtol=1e-4, atol=at * abs(want_c[1]) + 1e-9), f"D {k}: {checksum(D[k])} vs {want_c}"


def test_content_loss_oracle_vs_pinned_torchvision_values(golden_dir):
    """Row A7's pin, when available (tools/pin_vgg.py; skipped in the build container: no torchvision / ImageNet weights): the oracle's
    VGG-19 restatement on the ImageNet weights against the values the reference's ContentLoss produced (BSRGAN/model.py:536-554: five
    detached L1 values; ESRGAN/model.py:281-292: one differentiable value + d/dSR), 1e-5.  Also settles the in-place-ReLU question of
    SURVEY 8a/A7: the fixture records whether each tap held negative values."""
    g, sd, _ = pinned_vgg(golden_dir)
    nodes, mean, std = [str(n) for n in g["nodes"]], [float(v) for v in g["mean"]], [float(v) for v in g["std"]]
    sr, gt = torch.tensor(g["sr"]), torch.tensor(g["gt"])
    post = {n: not bool(g[f"tap_stats/{n}"][2]) for n in nodes}
    assert post == {n: n != nodes[-1] for n in nodes}, f"tap semantics differ from SURVEY's reading (post-ReLU except the last): {post}"
    got = O.content_loss(sr, gt, sd, nodes, mean, std, taps_post_relu=True)
    assert np.allclose(got.numpy(), g["bsrgan_values"], rtol=1e-5, atol=1e-7), (got.numpy(), g["bsrgan_values"])
    s1 = sr.clone().requires_grad_(True)
    v1 = O.content_loss_single(s1, gt, sd, "features.34", mean, std)
    v1.backward()
    assert abs(v1.item() - float(g["esrgan_value"])) < 1e-5 * abs(float(g["esrgan_value"]))
    ref = torch.tensor(g["esrgan_dsr"])
    assert ((s1.grad - ref).norm() / ref.norm()).item() < 1e-4
