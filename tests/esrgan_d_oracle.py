"""Torch-CPU restatement, in float64, of the two graphs whose backward passes every ESRGAN GAN step runs besides the generator's: the
BatchNorm discriminator (ESRGAN/model.py:88-141; oracle/srgan_oracle.esrgan_discriminator_forward in training mode plus autograd) and
the differentiable single-node VGG content loss (ESRGAN/model.py:258-292; oracle/srgan_oracle.content_loss_single plus autograd for
d/dSR).  The checker of tests/test_esrgan_d_host.py and of the oracle tests in tests/test_esrgan_d_gpu.py, in the style of
tests/bsrgantrans_oracle.py.  The layer tables are oracle/srgan_oracle.py's (ESRGAN_D_CONVS, ESRGAN_D_STRIDES, vgg19_feature_layers).

    discriminator(x, state, ...)             logits, the eleven stored activations, batch statistics, running statistics, dx, 33 gradients
    content_loss(sr, gt, P, node, ...)       the loss and d/dSR
    all_runs(graph, *args, **kw)             the four runs "f64", "f32", "f16", "bf16" of either

Switches of both, as in tests/bsrgantrans_oracle.py:
  dtype    torch.float64 (the oracle) or torch.float32 (its gap to the float64 run is the yardstick G of the exact-fp32 mode).
  emulate  None, torch.float16 or torch.bfloat16: rounds to that type exactly where the HIP engine stores that type.  Its gap to the
           plain float64 run is the yardstick E of the 16-bit modes.
           Discriminator (sr_gan_fd_amd/engine_e.py, csrc/norm.hip): forward -- the image (sp.xin), every packed conv / linear weight,
           every conv output y_i the BatchNorm reads, every LeakyReLU output a_i and f1; biases, gamma / beta, the statistics (fp32 sums
           over the STORED y_i) and the logits are fp32.  Backward -- the logits' gradient (sp.dl), df1 (at f1's pre-activation: the
           LeakyReLU' mask is the epilogue of the conv that writes it), dA_i (at a_i: bn_partial_kernel and chan_affine_kernel apply
           LeakyReLU' in fp32 to the stored dA_i, and the BatchNorm backward's sums are fp32 over that product and the stored y_i), dY_i
           (at y_i), and stage 1's dAp (at a0's pre-activation: a0's mask is that launch's epilogue).  Weight gradients -- fp32 sums over
           the stored tensors -- and the image's gradient (sp.dxp) are fp32.
           Content loss (sr_gan_fd_amd/engine_v.py): forward -- the normalised image, every packed weight, every conv(+ReLU) output and
           the tap map; the loss is an fp32 sum over the stored halves.  Backward -- g_tap (at the tap map) and every ``gin``: a conv's
           data gradient is stored after the ReLU' mask of its input (at that ReLU's pre-activation) or, where its input is a pooled
           map, as it is (at the pool's output), and the pool's backward writes the routed, masked copy (at the pre-activation too);
           the image's gradient (sp.dxp) is fp32 and 1/std is applied to it at the end.
  signs / states   None, or the discrete states the DERIVATIVES take in place of this run's own; the forward stays the plain op.  A
           LeakyReLU / ReLU input within a rounding of zero, two window elements within a rounding of each other, a tap difference within
           a rounding of zero have one state in float64 and may have the other in a 16-bit run, and the derivative then differs by a
           factor of 5 (or all of it).  Replaying the pattern a 16-bit run stored takes those few units out of the comparison.
           ``signs``: one boolean tensor per LeakyReLU in forward order (a0, a1 ... a9, f1).  ``states``: {"relu": one boolean tensor per
           ReLU of the SR half in forward order, "route": per max-pool the index 0..3 (row-major in the 2 x 2 window) of the element
           that receives the gradient, "sign": sign(sr_f - gt_f) in {-1, 0, 1}}.
  loss_scale   the backward pass runs on gradients multiplied by it (every rounded adjoint carries it, as under the f16 GradScaler) and
           the results are divided by it at the end.
  probe    a dict that receives "pre": every LeakyReLU pre-activation (discriminator) / every stored map (content loss: "maps").
  mutate   (discriminator) None, or one deliberate error for tests/test_esrgan_d_host.py's "the bound sees it" checks -- see MUTATIONS.
"""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import srgan_oracle as O

SLOPE, EPS, MOMENTUM = 0.2, 1e-5, 0.1
F16_LOSS_SCALE = 65536.0                             # the f16 backward runs loss-scaled (tests/test_esrgan_d_gpu.py, the trainers' GradScaler)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "esrgan_discriminator.npz")
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
NODE = "features.34"
# name: what ``mutate={name: stage}`` does to stage 1..9 of the discriminator.  (The content loss's derivatives are all in ``states``: its
# mutations are edits of them, tests/test_esrgan_d_host.py.)
MUTATIONS = {
    "slope": "LeakyReLU' of that stage's backward takes 0.25 for 0.2",
    "rstd_const": "that stage's BatchNorm backward treats rstd as a constant",
    "eps": "that stage's BatchNorm adds 1e-3 for 1e-5",
    "unbiased": "that stage's BatchNorm normalises with the unbiased variance",
}


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
    """LeakyReLU(0.2) whose derivative takes the pattern ``positive`` instead of the input's own, and ``slope`` where it is not set"""
    @staticmethod
    def forward(ctx, t, positive, slope):
        ctx.slope = slope
        ctx.save_for_backward(positive)
        return F.leaky_relu(t, SLOPE)

    @staticmethod
    def backward(ctx, g):
        one = torch.ones((), dtype=g.dtype)                          # (python scalars would make the slope a float32 number)
        return g * torch.where(ctx.saved_tensors[0], one, ctx.slope * one), None, None


class _ReLUMask(torch.autograd.Function):
    """ReLU whose derivative is 1 where ``positive`` says so"""
    @staticmethod
    def forward(ctx, t, positive):
        ctx.save_for_backward(positive)
        return F.relu(t)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0].to(g.dtype), None


def windows(t):
    """(N, C, H, W) -> (N, C, H/2, W/2, 4): the 2 x 2 windows, their elements in row-major order"""
    n, c, h, w = t.shape
    return t.view(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4)


def unwindows(t):
    n, c, ho, wo, _ = t.shape
    return t.view(n, c, ho, wo, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, 2 * ho, 2 * wo)


class _MaxPoolRoute(torch.autograd.Function):
    """2 x 2 max-pool whose gradient goes to window element ``route`` (0..3, row-major)"""
    @staticmethod
    def forward(ctx, t, route):
        ctx.save_for_backward(route)
        return F.max_pool2d(t, 2, 2)

    @staticmethod
    def backward(ctx, g):
        route, = ctx.saved_tensors
        return unwindows(F.one_hot(route, 4).to(g.dtype) * g.unsqueeze(-1)), None


class _L1Sign(torch.autograd.Function):
    """mean |a - b| whose derivative w.r.t. a is ``sign`` / numel"""
    @staticmethod
    def forward(ctx, a, b, sign):
        ctx.save_for_backward(sign)
        return (a - b).abs().mean()

    @staticmethod
    def backward(ctx, g):
        sign, = ctx.saved_tensors
        return g * sign.to(g.dtype) / sign.numel(), None, None


# ---- the states as the kernels derive them from a stored map ----
def positive(stored):
    """csrc/norm.hip (bn_partial_kernel, chan_affine_kernel): ``av[q] > 0.f ? 1.f : act_slope``; csrc/conv_igemm.hip's mask epilogue:
    ``to_f(mg[...]) > 0.f ? 1.f : a.mask_slope`` -- on the STORED activation"""
    return stored > 0


def pool_route(stored, last=False):
    """csrc/resample.hip, maxpool2_relu_bwd_kernel: the first maximum of the window in row-major order (``if (v > best)``); the gradient
    is zero where that maximum is not positive, which the ReLU mask of the same stored map says too.  ``last``: the last maximum (the
    "route_last" mutation)."""
    w = windows(stored)
    best, arg = w[..., 0], torch.zeros(w.shape[:-1], dtype=torch.long)
    for j in (1, 2, 3):
        take = (w[..., j] >= best) if last else (w[..., j] > best)
        best, arg = torch.where(take, w[..., j], best), torch.where(take, torch.full_like(arg, j), arg)
    return arg


def l1_sign(a, b):
    """csrc/loss.hip, l1_grad_views_kernel: ``d > 0.f ? sc : (d < 0.f ? -sc : 0.f)`` of the difference of the stored halves"""
    return torch.sign(a - b)


def rel_l2(a, ref):
    a, ref = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    return float((a - ref).norm() / (ref.norm() + 1e-300))


# ---- the discriminator ----
ACTS = ["a%d" % i for i in range(10)] + ["f1"]


def d_param_names(state):
    return [k for k in state if k.endswith((".weight", ".bias"))]


def bce_ones(logits):
    """BCEWithLogitsLoss against ones, mean"""
    return O.bce_with_logits_mean(logits, 1.0)


def discriminator(x, state, dtype=torch.float64, emulate=None, signs=None, d_logits=None, loss=None, loss_scale=1.0, probe=None, mutate=None):
    """x (N, 3, 128, 128); state: the module's state dict before the pass.  ``d_logits`` (the logits' gradient) or ``loss`` (a function of
    the logits, e.g. ``bce_ones``) starts the backward pass; with neither, forward only.  Returns {"logits"; "act.a0" .. "act.a9",
    "act.f1"; "bn.mean.i", "bn.var.i" (biased), "bn.rstd.i" for the stages i = 1..9; "state.<key>": the running statistics and batch
    counters after the pass; with a backward pass "loss" (if given), "dx" and "grad.<parameter>" for all 33}."""
    em, mut = emulate, mutate or {}
    back = d_logits is not None or loss is not None
    names = d_param_names(state)
    P = {k: state[k].detach().to(dtype).clone().requires_grad_(back) for k in names}
    xl = x.detach().to(dtype).clone().requires_grad_(back)
    res, pre_all = {}, []

    def act(pre, k, at_pre):
        """LeakyReLU number ``k`` and its stored output.  at_pre: the stored adjoint is the one of the pre-activation (the mask is the
        epilogue of the launch that writes it); else the one of the output (the BatchNorm backward reads it and applies the mask in fp32)"""
        pre_all.append(pre.detach())
        slope = 0.25 if mut.get("slope") == k else SLOPE
        t = _r(pre, em, fwd=False, bwd=True) if at_pre else pre
        if signs is None and slope == SLOPE:
            a = F.leaky_relu(t, SLOPE)
        else:
            a = _LeakyReLUSigns.apply(t, (pre.detach() > 0) if signs is None else signs[k], slope)
        return _r(a, em, bwd=not at_pre)

    h = _r(xl, em)
    for i, (fi, st) in enumerate(zip(O.ESRGAN_D_CONVS, O.ESRGAN_D_STRIDES)):
        w = _r(P["features.%d.weight" % fi], em)
        if i == 0:
            h = act(F.conv2d(h, w, P["features.0.bias"], stride=st, padding=1), 0, True)
        else:
            b = "features.%d" % (fi + 1)
            y = _r(F.conv2d(h, w, None, stride=st, padding=1), em, bwd=True)
            n = y.numel() / y.shape[1]
            mean, var = y.mean(dim=(0, 2, 3)), y.var(dim=(0, 2, 3), unbiased=False)
            rstd = 1.0 / torch.sqrt((var * n / (n - 1) if mut.get("unbiased") == i else var) + (1e-3 if mut.get("eps") == i else EPS))
            res["bn.mean.%d" % i], res["bn.var.%d" % i], res["bn.rstd.%d" % i] = mean.detach(), var.detach(), rstd.detach()
            res["state." + b + ".running_mean"] = (1 - MOMENTUM) * state[b + ".running_mean"].to(dtype) + MOMENTUM * mean.detach()
            res["state." + b + ".running_var"] = (1 - MOMENTUM) * state[b + ".running_var"].to(dtype) + MOMENTUM * var.detach() * n / (n - 1)
            res["state." + b + ".num_batches_tracked"] = state[b + ".num_batches_tracked"] + 1
            if mut.get("rstd_const") == i:
                rstd = rstd.detach()
            pre = (y - mean[None, :, None, None]) * (rstd * P[b + ".weight"])[None, :, None, None] + P[b + ".bias"][None, :, None, None]
            h = act(pre, i, False)
        res["act.a%d" % i] = h.detach()
    f1 = act(F.linear(torch.flatten(h, 1), _r(P["classifier.0.weight"], em), P["classifier.0.bias"]), 10, True)
    res["act.f1"] = f1.detach()
    logits = F.linear(f1, _r(P["classifier.2.weight"], em), P["classifier.2.bias"])
    res["logits"] = logits.detach()
    if probe is not None:
        probe["pre"] = pre_all
    if back:
        out = _r(logits, em, fwd=False, bwd=True)                    # sp.dl
        if loss is not None:
            value = loss(out)
            res["loss"] = value.detach()
            (value * loss_scale).backward()
        else:
            out.backward(d_logits.to(dtype) * loss_scale)
        res["dx"] = xl.grad / loss_scale
        for k in names:
            res["grad." + k] = P[k].grad / loss_scale
    return res


def stored_signs(res):
    """``signs`` of a run, from its stored activations, by the kernels' predicate"""
    return [positive(res["act." + k]) for k in ACTS]


# ---- the content loss ----
def vgg_chain(node=NODE):
    """[("conv", idx, followed by a ReLU) | ("pool", idx, None)] up to the node"""
    last = int(node.split(".")[1])
    return [(kind, idx, idx != last if kind == "conv" else None) for kind, idx, _ in O.vgg19_feature_layers() if idx <= last and kind != "relu"]


def content_loss(sr, gt, P, node=NODE, mean=MEAN, std=STD, dtype=torch.float64, emulate=None, states=None, upstream=1.0, loss_scale=1.0,
                 probe=None):
    """Returns {"feat_sr", "feat_gt": the two halves of the stored tap map, "loss": mean |feat_sr - feat_gt|, "dsr": d(upstream * loss)/d sr}.
    ``probe`` receives "maps": the stored map
    of the SR half after every ReLU and, last, the tap map; "pre_pool": the stored SR maps the pools read; "feat_gt": the GT's tap map; "pre": every ReLU's
    pre-activation of the SR half."""
    em = emulate
    m, s = torch.tensor(mean, dtype=dtype).view(1, 3, 1, 1), torch.tensor(std, dtype=dtype).view(1, 3, 1, 1)
    W = {k: v.detach().to(dtype) for k, v in P.items()}
    chain = vgg_chain(node)
    maps, pre_pool, pres = [], [], []

    def run(img, grad):
        h = _r((img - m) / s, em)
        n_relu = n_pool = 0
        for kind, idx, relu in chain:
            if kind == "conv":
                pre = F.conv2d(h, _r(W["features.%d.weight" % idx], em), W["features.%d.bias" % idx], padding=1)
                if not relu:
                    h = _r(pre, em, bwd=True)                         # the tap map, and g_tap
                elif not grad:
                    h = _r(F.relu(pre), em)
                else:
                    pres.append(pre.detach())
                    t = _r(pre, em, fwd=False, bwd=True)              # gin: stored after the mask
                    h = _r(F.relu(t) if states is None else _ReLUMask.apply(t, states["relu"][n_relu]), em)
                    n_relu += 1
                if grad:
                    maps.append(h.detach())
            elif not grad:
                h = F.max_pool2d(h, 2, 2)
            else:
                pre_pool.append(h.detach())
                h = F.max_pool2d(h, 2, 2) if states is None else _MaxPoolRoute.apply(h, states["route"][n_pool])
                h = _r(h, em, fwd=False, bwd=True)                    # the data gradient of the conv that reads the pooled map
                n_pool += 1
        return h
    srl = sr.detach().to(dtype).clone().requires_grad_(True)
    with torch.no_grad():
        fg = run(gt.detach().to(dtype), False)
    fs = run(srl, True)
    value = F.l1_loss(fs, fg) if states is None else _L1Sign.apply(fs, fg, states["sign"])
    (value * (upstream * loss_scale)).backward()
    if probe is not None:
        probe["maps"], probe["pre_pool"], probe["feat_gt"], probe["pre"] = maps, pre_pool, fg, pres
    return {"feat_sr": fs.detach(), "feat_gt": fg, "loss": value.detach(), "dsr": srl.grad / loss_scale}


def stored_states(probe):
    """``states`` of a run from the maps it stored (``probe``), by the kernels' rules"""
    return {"relu": [positive(t) for t in probe["maps"][:-1]], "route": [pool_route(t) for t in probe["pre_pool"]],
            "sign": l1_sign(probe["maps"][-1], probe["feat_gt"])}


# ---- the four runs ----
EMULATE = {"f64": None, "f32": None, "f16": torch.float16, "bf16": torch.bfloat16}


def run_kw(tag):
    """the switches of run ``tag``; the f16 run's backward is loss-scaled as the engine's is"""
    return dict(dtype=torch.float32 if tag == "f32" else torch.float64, emulate=EMULATE[tag], loss_scale=F16_LOSS_SCALE if tag == "f16" else 1.0)


def all_runs(graph, *args, tags=("f64", "f32", "f16", "bf16"), **kw):
    """{"f64", "f32", "f16", "bf16"} (or ``tags`` of them): ``graph`` (discriminator or content_loss) over the same arguments"""
    return {tag: graph(*args, **run_kw(tag), **kw) for tag in tags}


# ---- inputs ----
def build_discriminator():
    """the fixture's module: seed 0, BatchNorm weights and biases drawn as tests/golden's recipe draws them"""
    from sr_gan_fd_amd import model as M
    torch.manual_seed(0)
    d = M.discriminator()
    with torch.no_grad():
        for m in d.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.3, 0.3)
    return d


@functools.lru_cache(maxsize=None)
def d_inputs(n=2):
    """(the first ``n`` images of the fixture's x, the module's state before any pass)"""
    with np.load(FIXTURE) as z:
        x = torch.from_numpy(z["x"][:n]).float()
    return x, {k: v.detach().clone() for k, v in build_discriminator().state_dict().items()}


def build_content_loss(seed=3):
    """seeded BEFORE the module is constructed: nn.Conv2d's default initialisation draws from the global generator"""
    from sr_gan_fd_amd import model as M
    torch.manual_seed(seed)
    return M.ContentLoss(NODE, MEAN, STD)


@functools.lru_cache(maxsize=None)
def content_inputs():
    """(sr, gt, {"features.i.weight" / ".bias"}) at 2 x 3 x 48 x 32"""
    cl = build_content_loss()
    g = torch.Generator().manual_seed(3)
    sr, gt = torch.rand(2, 3, 48, 32, generator=g), torch.rand(2, 3, 48, 32, generator=g)
    return sr, gt, {"features." + k: v.detach().clone() for k, v in cl.features.state_dict().items()}
