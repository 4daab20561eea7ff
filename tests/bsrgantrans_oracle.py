"""Torch-CPU restatement of the reference's BSRGANtrans (A-ESRGAN/model.py:643-746) and of the two training iterations the reference's
scripts run around it, the checker of tests/test_bsrgantrans_host.py and tests/test_bsrgantrans_gpu.py.  Written from the reference's
behaviour; tests/golden/bsrgantrans.npz pins it to the reference's own float64 numbers.

    generator(x, state, upscale, ...)        forward, and with d_out the backward
    g_only_step(...), gan_step(...)          train_bsrnet.py:244-272 / train_aesrgan.py:396-483 around this forward, assembled from
                                             oracle/srgan_oracle.py's pieces (its gan_step has no hook for the generator)
Switches of ``generator``, as in tests/transformer_oracle.py (whose ``encoder`` is the block):
  dtype    torch.float64 (the oracle) or torch.float32 (its gap to the float64 run is the yardstick G of the exact-fp32 mode).
  emulate  None, torch.float16 or torch.bfloat16: rounds to that type exactly where the HIP engine stores that type
           (sr_gan_fd_amd/engine.py, engine_trans.py, transformer.py): the image; every conv weight (biases stay fp32); conv1's output;
           every growth conv's LeakyReLU output; every dense block's output (conv5, its scale and the one or two residuals are one
           epilogue: one rounding); the stride-2 conv's LeakyReLU output -- the block's input --; the block's own points;
           upsamplingTrans's, upsampling{1,2}'s and conv3's LeakyReLU outputs; conv2's output plus conv1's.  conv4's output is fp32.
           Gradients: a stored activation's adjoint is stored in the same type, taken at the layer's PRE-activation (the LeakyReLU'
           mask is applied in the epilogue of the conv that writes it) and summed over all its consumers before the one rounding; the
           SR's gradient is rounded after the clamp's derivative; the image's gradient and the parameters' are fp32.
           Its gap to the plain float64 run is the yardstick E of the 16-bit modes.
  masks    None (eval mode) or the module's ``dropout_masks()``: {"transformer_encoder.layers.{i}.<site>": uint8 keep-mask}; ``p``.
  probe    a dict that receives "pre" (every LeakyReLU pre-activation), "sr_pre" (conv4's output before the clamp), "enc_src" /
           "enc_out", the stored tensors "out1", "block" (every dense block's output), "ut", "f0" and "c3", transformer_oracle's
           probes of the block and, from a run with d_out, the stored adjoints "d_pre" (of every LeakyReLU pre-activation), "d_block" and
           "d_f0", each list in the order the backward pass reaches them.
"""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import srgan_oracle as O
from tests import transformer_oracle as TO

ENC = "transformer_encoder."
UNUSED = "transformer_layer."
NHEAD = 4                                            # hard-coded in the reference (model.py:673)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bsrgantrans.npz")


class _Round(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, emulate, fwd, bwd):
        ctx.emulate = emulate if bwd else None
        return t.to(emulate).to(t.dtype) if fwd else t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return (g if ctx.emulate is None else g.to(ctx.emulate).to(g.dtype)), None, None, None


def _r(t, emulate, fwd=True, bwd=False):
    return t if emulate is None else _Round.apply(t, emulate, fwd, bwd)


class _LeakyReLUSigns(torch.autograd.Function):
    """LeakyReLU(0.2) whose derivative takes the sign pattern ``positive`` instead of the input's own (forward_graph's ``signs``)"""
    @staticmethod
    def forward(ctx, t, positive):
        ctx.save_for_backward(positive)
        return F.leaky_relu(t, 0.2)

    @staticmethod
    def backward(ctx, g):
        return g * torch.where(ctx.saved_tensors[0], 1.0, 0.2).to(g.dtype), None


class _ClampSigns(torch.autograd.Function):
    """clamp to [0, 1] whose derivative is 1 where ``inside`` says so (forward_graph's ``signs``)"""
    @staticmethod
    def forward(ctx, t, inside):
        ctx.save_for_backward(inside)
        return torch.clamp(t, 0.0, 1.0)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0].to(g.dtype), None


class _Encoder(torch.autograd.Function):
    """tests/transformer_oracle.encoder as one node of the generator's graph: its own float64 / emulated forward, and in the backward
    its own autograd run from the incoming gradient (d src and the block's parameter gradients)"""
    @staticmethod
    def forward(ctx, src, cfg, names, *params):
        ctx.cfg, ctx.names = cfg, names
        ctx.save_for_backward(src, *params)
        state = dict(zip(names, params))
        return TO.encoder(src, state, NHEAD, dtype=cfg["dtype"], emulate=cfg["emulate"], masks=cfg["masks"], p=cfg["p"], probe=cfg["probe"])["out"]

    @staticmethod
    def backward(ctx, g):
        src, *params = ctx.saved_tensors
        cfg, state = ctx.cfg, dict(zip(ctx.names, params))
        with torch.enable_grad():
            res = TO.encoder(src, state, NHEAD, dtype=cfg["dtype"], emulate=cfg["emulate"], masks=cfg["masks"], p=cfg["p"], d_out=g)
        return (res["dsrc"], None, None) + tuple(res[k] for k in ctx.names)


def n_rrdb(state):
    return O.count_rrdb(state)


def forward_graph(x, P, upscale, dtype=torch.float64, emulate=None, masks=None, p=0.0, probe=None, signs=None):
    """the SR as a node of an autograd graph over the leaves ``P`` (state-dict keys) and ``x``.  ``signs``: None, or {"lrelu": one
    boolean tensor per LeakyReLU in forward order ("pre"'s order), "inside": which SR pixels lie strictly inside the clamp}: the pattern
    the DERIVATIVES take in the backward pass in place of this run's own -- the forward is untouched.  A pre-activation within a
    rounding of zero (an SR value within a rounding of 0 or 1) has one state in float64 and may have the other in a 16-bit run;
    replaying the pattern a GPU run stored takes those few units out of the comparison."""
    em, lrelus = emulate, []
    note = (lambda k, t: probe.setdefault(k, []).append(t.detach())) if probe is not None else (lambda k, t: None)

    def note_grad(k, t):
        """the stored adjoint of ``t`` (``t`` feeds the rounding point of its gradient), in the order the backward pass reaches them"""
        if probe is not None and t.requires_grad:
            t.register_hook(lambda g: probe.setdefault(k, []).append(g.detach()))
    conv = lambda t, name, stride=1: F.conv2d(t, _r(P[name + ".weight"], em), P[name + ".bias"], stride=stride, padding=1)

    def act(pre):
        """LeakyReLU whose output is stored, and whose adjoint is stored at the pre-activation"""
        note("pre", pre)
        note_grad("d_pre", pre)
        lrelus.append(None)
        t = _r(pre, em, fwd=False, bwd=True)
        return _r(F.leaky_relu(t, 0.2) if signs is None else _LeakyReLUSigns.apply(t, signs["lrelu"][len(lrelus) - 1]), em)
    up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")
    out1 = _r(conv(_r(x, em), "conv1"), em, bwd=True)
    note("out1", out1)
    cur = _r(out1, em, fwd=False, bwd=True)          # the trunk's share of conv1's adjoint is stored before conv2's is added to it
    for i in range(n_rrdb(P)):
        x_rrdb = cur
        for r in (1, 2, 3):
            pre, feats = "trunk.%d.rdb%d." % (i, r), [cur]
            for k in range(1, 5):
                feats.append(act(conv(torch.cat(feats, 1), pre + "conv%d" % k)))
            y = conv(torch.cat(feats, 1), pre + "conv5") * 0.2 + cur
            if r == 3:
                y = y * 0.2 + x_rrdb
            note_grad("d_block", y)
            cur = _r(y, em, bwd=True)
            note("block", cur)
    ds = act(conv(cur, "downsamplingTrans.0", stride=2))                     # (B, C, h, w)
    B, C, h, w = ds.shape
    src = ds.permute(0, 2, 3, 1).flatten(1, 2)                                # (B, h w, C), read as (S, N, E): the batch is the sequence axis
    names = tuple(k for k in P if k.startswith(ENC))
    sub = None if masks is None else {k[len(ENC):]: v for k, v in masks.items()}
    cfg = dict(dtype=dtype, emulate=em, masks=sub, p=p, probe=probe)
    enc = _Encoder.apply(src, cfg, tuple(k[len(ENC):] for k in names), *[P[k] for k in names])
    note("enc_src", src)
    note("enc_out", enc)
    t = enc.view(B, h, w, C).permute(0, 3, 1, 2)
    t = act(conv(up(t), "upsamplingTrans.0"))
    note("ut", t)
    y = conv(t, "conv2") + out1
    note_grad("d_f0", y)
    cur = _r(y, em, bwd=True)
    note("f0", cur)
    cur = act(conv(up(cur), "upsampling1.0"))
    if upscale == 4:
        cur = act(conv(up(cur), "upsampling2.0"))
    cur = act(conv(cur, "conv3.0"))
    note("c3", cur)
    pre = conv(cur, "conv4")
    note("sr_pre", pre)
    pre = _r(pre, em, fwd=False, bwd=True)
    return torch.clamp(pre, 0.0, 1.0) if signs is None else _ClampSigns.apply(pre, signs["inside"])


def param_names(state):
    return [k for k in state if k.endswith("weight") or k.endswith("bias")]


def leaves(state, dtype, grad=True):
    return {k: v.detach().to(dtype).clone().requires_grad_(grad) for k, v in state.items()}


def generator(x, state, upscale=2, dtype=torch.float64, emulate=None, masks=None, p=0.0, d_out=None, probe=None, signs=None):
    """x (B, 3, H, W); state: the module's state dict.  Returns {"out"} and, with d_out, also "dx" and one entry per parameter under its
    state-dict key: the gradient, or None for ``transformer_layer.*`` (registered by the reference, never called)."""
    P = leaves(state, dtype, d_out is not None)
    xl = x.detach().to(dtype).clone().requires_grad_(d_out is not None)
    out = forward_graph(xl, P, upscale, dtype, emulate, masks, p, probe, signs)
    res = {"out": out.detach()}
    if d_out is not None:
        out.backward(d_out.to(dtype))
        res["dx"] = xl.grad
        for k, v in P.items():
            res[k] = v.grad
            assert (v.grad is None) == k.startswith(UNUSED), k
    return res


def all_runs(x, state, upscale, d_out, masks=None, p=0.0, signs=None):
    kw = dict(masks=masks, p=p, d_out=d_out, signs=signs)
    return {"f64": generator(x, state, upscale, **kw), "f32": generator(x, state, upscale, dtype=torch.float32, **kw),
            "f16": generator(x, state, upscale, emulate=torch.float16, **kw), "bf16": generator(x, state, upscale, emulate=torch.bfloat16, **kw)}


def clamped(sr):
    """which SR pixels sit on the clamp"""
    return (sr <= 0.0) | (sr >= 1.0)


# ---- inputs: the fixture's recipe (tests/golden/make_golden_bsrgantrans.py) on this repository's seeded module ----
SEED, SCALE, BIAS, P_TRAIN = 5, 8.0, 0.5, 0.1
# name: (input shape, num_rrdb, upscale, construction seed) -- channels 64, growth 32 (nhead = 4: the smallest width with an attention
# kernel).  The seed is the fixture's, or the first from it on at which the oracle alone meets the host test's conditions (the two-RRDB
# network of seed 5 clamps 60 % of its SR).  Every case but the fixture's -- whose recipe is the reference run's -- has the q and k rows of
# both in_proj_weight multiplied by QK (and put back on the float16 grid), as tests/transformer_oracle.make_case doubles them: with the
# reference's initialisation the softmax rows are near uniform (mean entropy 0.98 .. 0.9995 of log B) and a wrong q / k gradient would
# hide in the tensor's norm; with QK they sit at 0.2 .. 0.9
QK = 5.0
CASES = {
    "fixture": ((3, 3, 6, 8), 1, 2, SEED),           # the fixture's shape
    "one_token": ((1, 3, 4, 4), 1, 2, SEED),         # one-token sequences, a 2 x 2 token map: the smallest the stride-2 conv can feed
    "odd_map": ((2, 3, 10, 6), 1, 2, SEED),          # token map 5 x 3: the parity classes have ragged edges
    "odd_batch": ((5, 3, 4, 6), 2, 2, SEED + 1),     # odd batch, and the second bucket marker
    "x4": ((2, 3, 4, 4), 1, 4, SEED),                # two tail stages, built through the class
}


def edit(module, qk=1.0):
    """the fixture's three edits, on a seeded module of the reference or of this repository; ``qk``: see QK"""
    with torch.no_grad():
        for prm in module.parameters():
            if prm.dim() == 4:
                prm.mul_(SCALE)
        module.conv4.bias.fill_(BIAS)
        for prm in module.transformer_encoder.parameters():
            prm.copy_(prm.to(torch.float16).float())
        if qk != 1.0:
            for layer in module.transformer_encoder.layers:
                w = layer.self_attn.in_proj_weight
                w[: 2 * w.shape[1]] = (w[: 2 * w.shape[1]] * qk).to(torch.float16).float()
    return module


def build_module(num_rrdb=1, upscale=2, seed=SEED, edited=True, qk=1.0):
    import contextlib
    import io
    from sr_gan_fd_amd import model as M
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        m = M.bsrgantrans_x2(num_rrdb=num_rrdb) if upscale == 2 else M.BSRGANtrans(num_rrdb=num_rrdb, upscale_factor=upscale)
    return edit(m, qk) if edited else m


def case_qk(name):
    return 1.0 if name == "fixture" else QK


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(x, state, d_out, upscale): the fixture's own input and gradient for "fixture", seeded ones of the same kind for the others"""
    shape, num_rrdb, upscale, seed = CASES[name]
    state = {k: v.detach().clone() for k, v in build_module(num_rrdb, upscale, seed, qk=case_qk(name)).state_dict().items()}
    if name == "fixture":
        with np.load(FIXTURE) as z:
            return torch.from_numpy(z["x"]).float(), state, torch.from_numpy(z["dsr"]).float(), upscale
    g = torch.Generator().manual_seed(100 + sorted(CASES).index(name))
    B, _, H, W = shape
    return torch.rand(*shape, generator=g), state, torch.randn(B, 3, H * upscale, W * upscale, generator=g), upscale


@functools.lru_cache(maxsize=None)
def eval_runs(name):
    """inputs and the four eval-mode oracle runs of a case, computed once and shared (nobody writes into them)"""
    x, state, d_out, upscale = case_inputs(name)
    probe = {}
    generator(x, state, upscale, probe=probe)
    return dict(x=x, state=state, d_out=d_out, upscale=upscale, probe=probe, **all_runs(x, state, upscale, d_out))


def make_masks(state, B, hw, p, seed):
    """CPU-drawn keep-masks under the module's keys (the host tests'; the GPU tests replay the module's own)"""
    sub = {k[len(ENC):]: v for k, v in state.items() if k.startswith(ENC)}
    return {ENC + k: v for k, v in TO.make_masks(sub, NHEAD, B, hw, p, seed).items()}


# ---- the two training iterations ----
def _loss_backward(loss, P, names):
    grads = torch.autograd.grad(loss, [P[k] for k in names], allow_unused=True)
    return dict(zip(names, grads))


def g_only_step(G, opt, ema, n_avg, lr_img, gt, *, upscale, lr, betas, eps, loss_weight=1.0, ema_decay=0.999, **fw):
    """train_bsrnet.py:244-272: forward, loss_weight * L1, backward, Adam (a parameter without a gradient is skipped), EMA.  ``G`` is
    updated in place; ``fw``: generator's dtype / emulate / masks / p.  Returns (loss, sr, n_averaged)."""
    names = param_names(G)
    P = {k: (v.detach().requires_grad_(True) if k in names else v) for k, v in G.items()}
    sr = forward_graph(lr_img.to(fw.get("dtype", torch.float64)), P, upscale, **fw)
    loss = loss_weight * O.l1_mean(sr, gt.to(sr.dtype))
    grads = _loss_backward(loss, P, names)
    with torch.no_grad():
        O.adam_step(G, grads, opt, lr, betas, eps)
    return float(loss), sr.detach(), O.ema_update(ema, G, n_avg, ema_decay)


def gan_step(G, D, g_opt, d_opt, ema, n_avg, lr_img, gt, *, upscale, g_lr, d_lr, betas, eps, pixel_weight, adversarial_weight,
             ema_decay=0.999, **fw):
    """train_aesrgan.py:396-483 with the content term off (oracle/srgan_oracle.gan_step's statements around this generator and
    aesrgan_unet_forward): D(gt) and D(sr.detach()) backward, D's Adam step, then pixel + adversarial loss through the UPDATED D, G's Adam
    step, EMA.  ``G`` and ``D`` are updated in place.  Returns the logged scalars, "sr" and "n_averaged"."""
    dt = fw.get("dtype", torch.float64)
    gn, dn = param_names(G), O.d_param_names(D)
    for k in dn:
        D[k] = D[k].detach().requires_grad_(True)
    P = {k: (v.detach().requires_grad_(True) if k in gn else v) for k, v in G.items()}
    gt = gt.to(dt)
    gt_out = O.aesrgan_unet_forward(gt, D, training=True)
    d_loss_hr = O.bce_with_logits_mean(gt_out, 1.0)
    g_hr = torch.autograd.grad(d_loss_hr, [D[k] for k in dn])
    sr = forward_graph(lr_img.to(dt), P, upscale, **fw)
    sr_out = O.aesrgan_unet_forward(sr.detach().clone(), D, training=True)
    d_loss_sr = O.bce_with_logits_mean(sr_out, 0.0)
    g_sr = torch.autograd.grad(d_loss_sr, [D[k] for k in dn])
    with torch.no_grad():
        O.adam_step(D, {k: a + b for k, a, b in zip(dn, g_hr, g_sr)}, d_opt, d_lr, betas, eps)
    for k in dn:
        D[k] = D[k].detach()
    pixel = pixel_weight * O.l1_mean(sr, gt)
    adv_out = O.aesrgan_unet_forward(sr, D, training=True)
    adv = adversarial_weight * O.bce_with_logits_mean(adv_out, 1.0)
    grads = _loss_backward(pixel + adv, P, gn)
    with torch.no_grad():
        O.adam_step(G, grads, g_opt, g_lr, betas, eps)
    return {"d_loss_hr": float(d_loss_hr), "d_loss_sr": float(d_loss_sr), "pixel_loss": float(pixel), "adversarial_loss": float(adv),
            "d_gt_probability": float(torch.sigmoid(gt_out.detach()).mean()), "d_sr_probability": float(torch.sigmoid(sr_out.detach()).mean()),
            "sr": sr.detach(), "n_averaged": O.ema_update(ema, G, n_avg, ema_decay)}


def rel_l2(a, ref):
    return TO.rel_l2(a, ref)
