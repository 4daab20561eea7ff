"""Torch-CPU restatement of the reference's SelfAttention (BSRGAN/model.py:388-402: nn.MultiheadAttention over the h*w positions of
every image, no masks, no dropout), the checker of tests/test_attention_host.py and tests/test_attention_gpu.py.

Two switches:
  dtype    torch.float64 (the oracle) or torch.float32 (the same statements in single precision: its gap to the float64 run is the
           yardstick G of the exact-fp32 mode).
  emulate  None, torch.float16 or torch.bfloat16: rounds x, both weight matrices, qkv, P (for P v only: the weights result is
           the mean of the unrounded probabilities) and O to that type -- where the HIP path rounds -- and leaves everything else in
           ``dtype``.  Its gap to the plain float64 run is the yardstick E of the 16-bit modes.

Gradients are torch autograd's over these statements.  A rounding point passes the gradient through unchanged, except at qkv and O,
whose adjoints (d qkv, dO) the HIP path also keeps in the 16-bit type: there the gradient is rounded as well.
"""
import math

import torch

PARAMS = ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias")
PREFIX = "multihead_attention."


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


def self_attention(x, state, num_heads, dtype=torch.float64, emulate=None, d_out=None):
    """x (b, c, h, w); state: the module's state dict (keys with or without the ``multihead_attention.`` prefix).
    Returns {"out": (b, c, h, w), "weights": (b, hw, hw)} and, with d_out (b, c, h, w), also "dx" and one gradient per parameter
    under its state-dict key without the prefix."""
    p = {k[len(PREFIX):] if k.startswith(PREFIX) else k: v for k, v in state.items()}
    leaves = {k: p[k].detach().to(dtype).clone().requires_grad_(d_out is not None) for k in PARAMS}
    xl = x.detach().to(dtype).clone().requires_grad_(d_out is not None)
    b, c, h, w = xl.shape
    L, H, D = h * w, num_heads, c // num_heads
    tok = _rnd(xl, emulate).flatten(2).transpose(1, 2)                                    # (b, L, c)
    qkv = _rnd(tok @ _rnd(leaves["in_proj_weight"], emulate).t() + leaves["in_proj_bias"], emulate, True)
    q, k, v = (t.reshape(b, L, H, D).transpose(1, 2) for t in qkv.split(c, dim=-1))       # (b, H, L, D)
    s = (q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(D))
    prob = torch.softmax(s, dim=-1)
    o = _rnd(_rnd(prob, emulate) @ v, emulate, True)                                      # (b, H, L, D)
    o = o.transpose(1, 2).reshape(b, L, c)
    out = (o @ _rnd(leaves["out_proj.weight"], emulate).t() + leaves["out_proj.bias"]).transpose(1, 2).reshape(b, c, h, w)
    res = {"out": out.detach(), "weights": prob.mean(dim=1).detach()}
    if d_out is not None:
        out.backward(d_out.to(dtype))
        res["dx"] = xl.grad
        for kname in PARAMS:
            res[kname] = leaves[kname].grad
    return res


def make_case(channels, num_heads, b, h, w, seed):
    """The input recipe of the attention tests: x ~ N(0, 1); nn.MultiheadAttention's seeded initial values with the q and k rows of
    in_proj_weight multiplied by 4 and both biases ~ N(0, 0.1) -- a peaked softmax, under which a mis-indexed key or head moves the
    result by the order of its magnitude; the incoming gradient ~ N(0, 1) in steps of 1/8.  Every value lies on the float16 grid, so a
    fixture can hold it in that type, and the gradient on bfloat16's too (the HIP path's copy of it in the compute type is exact).
    Returns (x, state dict with the module's keys, d_out)."""
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    mha = torch.nn.MultiheadAttention(channels, num_heads)
    with torch.no_grad():
        mha.in_proj_weight[: 2 * channels].mul_(4.0)
        mha.in_proj_bias.copy_(torch.randn(3 * channels, generator=g) * 0.1)
        mha.out_proj.bias.copy_(torch.randn(channels, generator=g) * 0.1)
    grid = lambda t: t.to(torch.float16).to(torch.float32)
    state = {PREFIX + k: grid(v.detach()) for k, v in mha.state_dict().items()}
    x = grid(torch.randn(b, channels, h, w, generator=g))
    d_out = torch.round(torch.randn(b, channels, h, w, generator=g) * 8.0) / 8.0
    return x, state, d_out


def peakedness(weights):
    """mean row maximum of the head-averaged weights times L (1 for a uniform softmax)"""
    return float(weights.max(dim=-1).values.mean()) * weights.shape[-1]


# name: (channels, heads, [(b, h, w), ...])
CASES = {
    "A": (256, 8, [(2, 6, 6)]),                      # one ragged key tile past 32
    "B": (512, 8, [(2, 9, 9)]),                      # D = 64, L odd, crosses 64
    "C": (64, 4, [(37, 2, 4)]),                      # D = 16, a sequence shorter than any tile, many batches
    "D": (256, 8, [(1, 10, 13)]),                    # more than two key tiles, ragged, h != w
    "E": (256, 8, [(2, 8, 8), (1, 16, 16)]),         # exact tile multiples, several query tiles
}
CASE_IDS = [(name, i) for name, (_, _, shapes) in CASES.items() for i in range(len(shapes))]


def case_inputs(name, i=0):
    c, heads, shapes = CASES[name]
    return (c, heads) + make_case(c, heads, *shapes[i], seed=1000 + 16 * sorted(CASES).index(name) + i)
