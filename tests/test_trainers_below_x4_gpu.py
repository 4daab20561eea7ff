"""The fused trainers over Real-ESRGAN's RRDBNet below x4 (Real_ESRGAN/model.py:190-204,248-262: PixelUnshuffle(2) at x2, (4) at x1 in
front of conv1, both nearest-x2 stages) against the fp32 CPU oracle's steps with the same ``unshuffle``.

Every case builds ``RRDBNet(num_rrdb=2, upscale_factor=s)`` with the suite's init recipe (``scaled_init(gen, 3.0, 0.5)``), runs two
iterations of the fused trainer and of the oracle's step function from the same weights on the same batches (batch 2), and compares
after each iteration.  The LR sizes put the dense blocks at small and ragged trunk sizes, where tiles go wrong: at x2 16x24 and 6x10
(the golden's odd case), at x1 4x4 (smaller than one 32-pixel tile row), 6x10 and -- generator-only, no discriminator to need sides that
are multiples of 8 -- 5x9.  The relativistic trainer runs at the 128x128 GT its BatchNorm discriminator's classifier fixes.

Every trainer gets ``eps=1e-4``: with Adam's default 1e-8 the first step moves an element whose gradient is within rounding noise of
zero (zero-initialised biases deep in the trunk) by +-lr whichever way the noise points, in the oracle's arithmetic as much as in the
kernels', and a per-element parameter comparison would measure that noise instead of the kernels.

Bounds.  float32 (the parity mode): logged scalars and SR within 1e-5 relative, and the module's own forward ``gen(lr)`` (run before the
first iteration, on the same weights) equal to the trainer's first SR within 1e-5 -- a path that unshuffles twice or not at all cannot
meet that.  Parameters after each iteration: every tensor of G and D within a bound of the largest magnitude of its network's parameters
(1e-5 for the generator-only trainer).  Measured against each tensor's OWN max-abs the error reaches 2e-2 (zero-initialised biases,
whose values after two steps are the Adam updates of gradients near eps; a LeakyReLU pre-activation within an fp32 rounding of zero flips
one mask and moves one channel's gradient by ~1 %) and 1.5 for the relativistic discriminator's BatchNorm biases (their gradients are
rounding noise: Adam turns them into +-lr steps of either sign), so no bound of 1e-3 or less can be written on that measure.
The relativistic trainer's discriminator side is looser: BatchNorm over two images amplifies one rounding of the logits.
float16 (the reference's autocast dtype) is held to the bounds of the config-crop f16 tests: scalars within 1e-3 relative (the
relativistic trainer's discriminator-side scalars within 5e-3, as its config-crop test), SR within 1e-3, probed parameters within 5e-3 of
their range, and no skipped optimizer step.  After its first discriminator update the relativistic trainer's discriminator-side scalars
are reported, not asserted: that Adam step moves the logits by ~3.6 (the 819k classifier weights all step +-lr) and its f16 sign noise
shows up as 6e-3 / 6e-2 relative (x2 / x1) in those scalars, while SR, pixel loss and probed parameters stay within their bounds.

Measured on the MI355X, worst over both iterations and the shapes of each trainer (f32: scalars / SR / parameters of the network's range;
f16: scalars / SR / probed parameters):
  GeneratorTrainer           f32 1.2e-7 / 2.3e-7 / 3.2e-7           f16 4.8e-7 / 3.4e-5 / 9.6e-5
  GanTrainer (BSRGAN order)  f32 2.0e-6 / 1.2e-6 / 4.2e-5           f16 3.4e-4 / 7.7e-5 / 6.7e-4
  GanTrainer (Real-ESRGAN)   f32 2.1e-7 / 1.2e-6 / 7.0e-6           f16 6.7e-5 / 4.2e-5 / 8.6e-4
  EsrganGanTrainer           f32 pixel 9.4e-8, D side 7.6e-4 / 3.4e-5 / 3.3e-4
                             f16 pixel 2.2e-6, D side (first iteration) 9.7e-4 / 5.8e-4 / 1.8e-3
  module forward vs the trainer's first SR (f32): 0 (identical bits) in every case.
The 4x4 and 5x9 trunks run: no kernel refuses them.
"""
import pytest
import torch

from tests.util import scaled_init, sd_to_params

pytestmark = pytest.mark.gpu

# float32 bounds per trainer; where one is above 1e-5 it is within 10x of what was measured (module docstring), never above 1e-3
F32 = dict(scalar=1e-5, d_scalar=1e-5, sr=1e-5)
F32_PARAMS = {"generator": 1e-5, "gan": 2e-4, "realesrgan": 5e-5, "esrgan": 1e-3}
F32_ESRGAN = dict(d_scalar=1e-3, sr=3e-4)
F16 = dict(scalar=1e-3, d_scalar=5e-3, sr=1e-3, probe=5e-3)

# (trainer, s, LR size): trunk sizes LR / (4 / s)
CASES = [("generator", 2, (32, 48)), ("generator", 2, (12, 20)), ("generator", 1, (16, 16)), ("generator", 1, (24, 40)),
         ("generator", 1, (20, 36))]
CASES += [(kind, s, hw) for kind in ("gan", "realesrgan") for s, hw in ((2, (32, 48)), (2, (12, 20)), (1, (16, 16)), (1, (24, 40)))]
CASES += [("esrgan", 2, (64, 64)), ("esrgan", 1, (128, 128))]

G_PROBES = ("conv1.weight", "conv4.bias")
D_PROBE = {"gan": "conv4.weight", "realesrgan": "conv4.weight", "esrgan": "features.0.weight"}


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def _build(kind, s, dtype):
    from sr_gan_fd_amd import model as M
    torch.manual_seed(0)
    d = None
    if kind in ("gan", "realesrgan"):
        d = M.discriminator_unet(in_channels=3, out_channels=1, channels=64)
    elif kind == "esrgan":
        d = M.discriminator()
    gen = M.RRDBNet(in_channels=3, out_channels=3, channels=64, growth_channels=32, num_rrdb=2, upscale_factor=s)
    scaled_init(gen, 3.0, 0.5)
    gen.compute_dtype = dtype
    if d is not None:
        d.compute_dtype = dtype
    return gen, d


def _trainer(kind, gen, d):
    from sr_gan_fd_amd.gan import GanTrainer
    from sr_gan_fd_amd.gan_esrgan import EsrganGanTrainer
    from sr_gan_fd_amd.trainer import GeneratorTrainer
    if kind == "generator":
        return GeneratorTrainer(gen, lr=1e-4, betas=(0.9, 0.99), eps=1e-4, ema_decay=0.999)
    if kind == "gan":               # bsrgan_config.py:137-159
        return GanTrainer(gen, d, None, g_lr=8e-5, d_lr=2e-4, betas=(0.9, 0.999), eps=1e-4, pixel_weight=20.0, content_weight=1.0,
                          adversarial_weight=0.5)
    if kind == "realesrgan":        # realesrgan_config.py:138-151
        return GanTrainer(gen, d, None, g_lr=1e-4, d_lr=1e-4, betas=(0.9, 0.99), eps=1e-4, pixel_weight=1.0,
                          content_weight=[0.1, 0.1, 1.0, 1.0, 1.0], adversarial_weight=0.1, generator_first=True)
    return EsrganGanTrainer(gen, d, None, eps=1e-4)


def _oracle_step(kind, G, D, g_opt, d_opt, lr, gt, gt_usm, u):
    """-> (scalars, sr) in the order _trainer_scalars() reads them"""
    from oracle import srgan_oracle as O
    if kind == "generator":
        loss, sr = O.g_only_step(G, g_opt, lr, gt, upscale=4, lr=1e-4, betas=(0.9, 0.99), eps=1e-4, unshuffle=u)
        return [loss], sr
    if kind == "gan":
        out = O.gan_step(G, D, g_opt, d_opt, lr, gt, upscale=4, g_lr=8e-5, d_lr=2e-4, betas=(0.9, 0.999), eps=1e-4, pixel_weight=20.0,
                         content_weight=1.0, adversarial_weight=0.5, unshuffle=u)
    elif kind == "realesrgan":
        out = O.realesrgan_gan_step(G, D, g_opt, d_opt, lr, gt, gt_usm, unshuffle=u)
    else:
        out = O.esrgan_gan_step(G, D, g_opt, d_opt, lr, gt, eps=1e-4, unshuffle=u)
    return [out[k] for k in ("d_loss", "pixel_loss", "adversarial_loss", "d_gt_probability", "d_sr_probability")], out["sr"]


def _trainer_scalars(kind, out):
    s = out.cpu().double().numpy()
    if kind == "generator":
        return [s[0]]
    if kind == "esrgan":            # [d_loss, pixel, content, adversarial, D(gt), D(sr)]
        return [s[0], s[1], s[3], s[4], s[5]]
    return [s[0] + s[1], s[2], s[3], s[4], s[5]]     # [d_loss_hr, d_loss_sr, pixel, adversarial, D(gt), D(sr)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("kind,s,hw", CASES, ids=[f"{k}-x{s}-{h}x{w}" for k, s, (h, w) in CASES])
def test_fused_trainer_below_x4_vs_oracle(kind, s, hw, dtype):
    from oracle import srgan_oracle as O
    u = 4 // s
    h, w = hw
    torch.manual_seed(9)
    batches = [(torch.rand(2, 3, h, w), torch.rand(2, 3, h * s, w * s), torch.rand(2, 3, h * s, w * s)) for _ in range(2)]
    gen, d = _build(kind, s, dtype)
    G = sd_to_params(gen.state_dict())
    g_opt = O.AdamState(G, O.g_param_names(G))
    D = d_opt = None
    if d is not None:
        D = {k: v.detach().clone() for k, v in d.state_dict().items()}
        d_opt = O.AdamState(D, [k for k in D if k.endswith((".weight", ".bias"))] if kind == "esrgan" else O.d_param_names(D))
        d = d.cuda().train()
    gen = gen.cuda().train()
    sr_module = None
    if dtype == torch.float32:
        with torch.no_grad():
            sr_module = gen(batches[0][0].cuda()).cpu()
    tr = _trainer(kind, gen, d)
    worst = dict(scalar=0.0, d_scalar=0.0, sr=0.0, params=0.0)
    d_after_update = own = 0.0            # reported only (see the module docstring)
    for it, (lr, gt, gt_usm) in enumerate(batches):
        want, want_sr = _oracle_step(kind, G, D, g_opt, d_opt, lr, gt, gt_usm, u)
        args = (lr.cuda(), gt.cuda()) + ((gt_usm.cuda(),) if kind == "realesrgan" else ())
        got = _trainer_scalars(kind, tr.step(*args))
        assert tr.sr.shape == gt.shape
        rel = [abs(a - b) / max(abs(b), 1e-6) for a, b in zip(got, want)]
        e_sr = _rel(tr.sr, want_sr)
        if kind == "esrgan":        # pixel loss, then the discriminator-side scalars
            worst["scalar"] = max(worst["scalar"], rel[1])
            if it == 1 and dtype == torch.float16:
                d_after_update = max(rel)
            else:
                worst["d_scalar"] = max(worst["d_scalar"], max(rel))
        else:
            worst["scalar"] = max(worst["scalar"], max(rel))
        worst["sr"] = max(worst["sr"], e_sr)
        if it == 0 and sr_module is not None:
            e_mod = _rel(tr.sr, sr_module)
            print(f"{kind} x{s} {h}x{w}: module forward vs trainer SR {e_mod:.2e}")
            assert e_mod < F32["sr"]
        if dtype == torch.float32:
            # every tensor, its error against the largest magnitude of its network's parameters
            nets = [(gen, G)] + ([(d, D)] if d is not None else [])
            e_p = {}
            for net, ref in nets:
                scale = max(ref[n].abs().max().item() for n, _ in net.named_parameters())
                for n, p in net.named_parameters():
                    e_p[n] = (p.detach().cpu().double() - ref[n].double()).abs().max().item() / scale
                    own = max(own, _rel(p, ref[n]))
        else:
            pairs = [(n, gen.get_parameter(n), G[n]) for n in G_PROBES]
            if d is not None:
                pairs.append((D_PROBE[kind], d.get_parameter(D_PROBE[kind]), D[D_PROBE[kind]]))
            e_p = {n: _rel(p, ref) for n, p, ref in pairs}
        n_worst = max(e_p, key=e_p.get)
        worst["params"] = max(worst["params"], e_p[n_worst])
        print(f"{kind} x{s} {h}x{w} {dtype} it{it}: scalars {['%.6g' % v for v in got]} vs {['%.6g' % v for v in want]} "
              f"rel {max(rel):.2e}; SR {e_sr:.2e}; worst parameter {n_worst} {e_p[n_worst]:.2e}")
    print(f"MEASURED {kind} x{s} {h}x{w} {dtype}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) +
          (f"; per tensor of its own max-abs {own:.2e}" if own else "") + (f"; D side after the D update {d_after_update:.2e}" if d_after_update else ""))
    if dtype == torch.float32:
        b = F32_ESRGAN if kind == "esrgan" else F32
        assert worst["scalar"] < F32["scalar"] and worst["d_scalar"] < b["d_scalar"], worst
        assert worst["sr"] < b["sr"] and worst["params"] < F32_PARAMS[kind], worst
    else:
        assert worst["scalar"] < F16["scalar"] and worst["d_scalar"] < F16["d_scalar"], worst
        assert worst["sr"] < F16["sr"] and worst["params"] < F16["probe"], worst
        rep = tr.scaler.report()
        assert rep["enabled"] and rep["skipped"] == 0 and rep["optimizer_steps"] == (2 if kind == "generator" else 4), rep
