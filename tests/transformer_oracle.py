"""Torch-CPU restatement of the reference's transformer block (A-ESRGAN/model.py:673-674, :725-726): a stack of post-norm
nn.TransformerEncoderLayer (ReLU, biases, LayerNorm eps 1e-5, no final norm, no masks) over a ``(S, N, E)`` tensor with
batch_first=False -- S is the sequence axis, every one of the N columns a sequence of its own.  The checker of
tests/test_transformer_host.py and tests/test_transformer_gpu.py.

Switches of ``encoder``:
  dtype    torch.float64 (the oracle) or torch.float32 (the same statements in single precision: its gap to the float64 run is the
           yardstick G of the exact-fp32 mode).
  emulate  None, torch.float16 or torch.bfloat16: rounds to that type where the HIP path stores that type (sr_gan_fd_amd/
           transformer.py lists the points): the input, the four weight matrices of a layer, qkv, P (once, before the keep-mask), O,
           the out-projection's output, z1, LayerNorm's y1, the hidden activation (again after its dropout, which the HIP path
           applies in place), linear2's output, z2 and y2.  LayerNorm normalises the ROUNDED z.  Its gap to the plain float64 run
           is the yardstick E of the 16-bit modes.
  masks    None (eval mode), or {"<layer prefix><site>": uint8 keep-mask} with the sites attn (N, heads, S, S), dropout1 (S, N, E),
           dropout (S, N, F) and dropout2 (S, N, E) and ``p`` the dropout probability: kept values are scaled by 1 / (1 - p).
           A site without a key has no dropout.

Gradients are torch autograd's over these statements.  A rounding point passes the gradient through unchanged where the HIP path
keeps no gradient in the 16-bit type (the input, the weights, P) and rounds it where it does (everything else above: the HIP path
stores the adjoint of each of those tensors in the compute type).  At z = x + dropout(r) the adjoint dz is stored twice, each rounded
once from the fp32 value: as the residual branch's gradient and, times the keep-mask, as r's.
"""
import functools
import math

import torch

LAYER_PARAMS = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
                "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")
SITES = ("attn", "dropout1", "dropout", "dropout2")
EPS = 1e-5


class _Round(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, emulate, round_grad):
        ctx.emulate = emulate if round_grad else None
        return t.to(emulate).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return (g if ctx.emulate is None else g.to(ctx.emulate).to(g.dtype)), None, None


def _rnd(t, emulate, round_grad=False):
    return t if emulate is None else _Round.apply(t, emulate, round_grad)


class _GradRound(torch.autograd.Function):
    """the identity, whose gradient is rounded: the residual branch of an add, whose adjoint (dz) the HIP path stores on its own"""
    @staticmethod
    def forward(ctx, t, emulate):
        ctx.emulate = emulate
        return t.clone()

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.emulate).to(g.dtype), None


def prefixes(state):
    """layer prefixes of a state dict: [""] for a lone layer, ["layers.0.", ...] for a stack"""
    if "linear1.weight" in state:
        return [""]
    n = 1 + max(int(k.split(".")[1]) for k in state if k.startswith("layers."))
    return ["layers.%d." % i for i in range(n)]


def layer_norm(z, gamma, beta):
    mu = z.mean(-1, keepdim=True)
    var = ((z - mu) ** 2).mean(-1, keepdim=True)                     # biased
    return (z - mu) / torch.sqrt(var + EPS) * gamma + beta, var


def encoder(src, state, nhead, dtype=torch.float64, emulate=None, masks=None, p=0.0, d_out=None, probe=None):
    """src (S, N, E); state: a lone layer's or a stack's state dict.  Returns {"out"} and, with d_out (S, N, E), also "dsrc" and one
    gradient per parameter under its state-dict key.  ``probe``: a dict that receives, per layer prefix, the softmax probabilities
    ("<pre>prob"), both LayerNorm variances ("<pre>var1", "<pre>var2") and the pre-dropout hidden activation ("<pre>hidden")."""
    grad = d_out is not None
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(grad) for k, v in state.items()}
    xl = src.detach().to(dtype).clone().requires_grad_(grad)
    S, N, E = xl.shape
    H, D = nhead, E // nhead
    masks, sc = masks or {}, 1.0 / (1.0 - p)
    R = lambda t, g=True: _rnd(t, emulate, g)
    RG = lambda t: t if emulate is None else _GradRound.apply(t, emulate)
    drop = lambda t, key: t * (masks[key].to(dtype).reshape(t.shape) * sc) if key in masks else t
    x = R(xl, False)
    for pre in prefixes(state):
        W = lambda name: R(leaves[pre + name], False)
        B = lambda name: leaves[pre + name]
        qkv = R(x @ W("self_attn.in_proj_weight").t() + B("self_attn.in_proj_bias"))              # (S, N, 3E)
        q, k, v = (t.reshape(S, N, H, D).permute(1, 2, 0, 3) for t in qkv.split(E, dim=-1))         # (N, H, S, D)
        prob = torch.softmax((q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(D)), dim=-1)              # (N, H, S, S)
        o = R(drop(R(prob, False), pre + "attn") @ v)                                               # (N, H, S, D)
        o = o.permute(2, 0, 1, 3).reshape(S, N, E)
        a = R(o @ W("self_attn.out_proj.weight").t() + B("self_attn.out_proj.bias"))
        z1 = R(RG(x) + drop(a, pre + "dropout1"), False)
        y1, var1 = layer_norm(z1, B("norm1.weight"), B("norm1.bias"))
        y1 = R(y1)
        hid = R(torch.relu(y1 @ W("linear1.weight").t() + B("linear1.bias")))
        f = R(R(drop(hid, pre + "dropout")) @ W("linear2.weight").t() + B("linear2.bias"))
        z2 = R(RG(y1) + drop(f, pre + "dropout2"), False)
        y2, var2 = layer_norm(z2, B("norm2.weight"), B("norm2.bias"))
        x = R(y2)
        if probe is not None:
            probe.update({pre + "prob": prob.detach(), pre + "var1": var1.detach(), pre + "var2": var2.detach(), pre + "hidden": hid.detach()})
    res = {"out": x.detach()}
    if grad:
        x.backward(d_out.to(dtype))
        res["dsrc"] = xl.grad
        for kname in state:
            res[kname] = leaves[kname].grad
    return res


def rel_l2(a, ref):
    """relative L2 distance, the measure of the module-level checks"""
    n = float(ref.double().norm())
    d = float((a.double() - ref.double()).norm())
    return d / n if n > 0 else (0.0 if d == 0 else float("inf"))


def make_case(E, heads, F, layers, S, N, seed):
    """The input recipe: src ~ N(0, 1); torch's seeded initial values of nn.TransformerEncoder with the q and k rows of every
    in_proj_weight multiplied by 2 (logits of standard deviation about 2: a softmax that is neither uniform nor one-hot, under which a
    mis-indexed key or head moves the result),
    every bias ~ N(0, 0.1), LayerNorm weights 1 + N(0, 0.1); the incoming gradient ~ N(0, 1) in steps of 1/8.  Every value lies on the
    float16 grid.  Returns (src, state dict with the stack's keys, d_out)."""
    import warnings
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        enc = torch.nn.TransformerEncoder(torch.nn.TransformerEncoderLayer(E, heads, F), layers, enable_nested_tensor=False)
    with torch.no_grad():
        for name, prm in enc.named_parameters():
            if name.endswith("in_proj_weight"):
                prm[: 2 * E].mul_(2.0)
            elif name.endswith("bias"):
                prm.copy_(torch.randn(prm.shape, generator=g) * 0.1)
            elif ".norm" in name:
                prm.copy_(1.0 + torch.randn(prm.shape, generator=g) * 0.1)
    grid = lambda t: t.to(torch.float16).to(torch.float32)
    state = {k: grid(v.detach()) for k, v in enc.state_dict().items()}
    src = grid(torch.randn(S, N, E, generator=g))
    d_out = torch.round(torch.randn(S, N, E, generator=g) * 8.0) / 8.0
    return src, state, d_out


def make_masks(state, heads, S, N, p, seed):
    """CPU-drawn keep-masks of every site of every layer (the host tests'; the GPU tests replay the module's own)"""
    g = torch.Generator().manual_seed(seed)
    E, F = state[prefixes(state)[0] + "linear1.weight"].shape[1], state[prefixes(state)[0] + "linear1.weight"].shape[0]
    shapes = {"attn": (N, heads, S, S), "dropout1": (S, N, E), "dropout": (S, N, F), "dropout2": (S, N, E)}
    return {pre + site: (torch.rand(shapes[site], generator=g) >= p).to(torch.uint8) for pre in prefixes(state) for site in SITES}


# name: (S, N, E, heads, hidden, layers) -- the smallest shapes at which the launches can go wrong
CASES = {
    "one_token": (1, 35, 64, 4, 96, 1),              # a single token per sequence: softmax over one key
    "odd_seq": (3, 35, 64, 4, 96, 1),                # odd sequence length, a token count that fills no tile
    "two_layers": (8, 130, 64, 4, 96, 2),            # the gradient between two layers, more than one workgroup everywhere
    "head32": (5, 35, 128, 4, 64, 1),                # head size 32: two lanes per row in the attention, 16 lanes per token in LayerNorm
    "ref_hidden": (8, 70, 64, 4, 2048, 2),           # the reference's hidden size and depth
}
P_TRAIN = 0.1
FIXTURE_CASES = ("ref",)                             # tests/golden/transformer.npz: captured from the reference's BSRGANtrans


def case_inputs(name):
    S, N, E, heads, F, layers = CASES[name]
    return (heads,) + make_case(E, heads, F, layers, S, N, seed=2000 + 16 * sorted(CASES).index(name))


@functools.lru_cache(maxsize=None)
def eval_runs(name):
    """inputs and the four eval-mode oracle runs of a case, computed once and shared (nobody writes into them)"""
    heads, src, state, d_out = case_inputs(name)
    return dict(heads=heads, src=src, state=state, d_out=d_out, **all_runs(src, state, heads, d_out))


def all_runs(src, state, heads, d_out, masks=None, p=0.0):
    kw = dict(masks=masks, p=p, d_out=d_out)
    return {"f64": encoder(src, state, heads, **kw), "f32": encoder(src, state, heads, dtype=torch.float32, **kw),
            "f16": encoder(src, state, heads, emulate=torch.float16, **kw), "bf16": encoder(src, state, heads, emulate=torch.bfloat16, **kw)}
