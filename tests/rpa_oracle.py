"""Torch-CPU restatement of A-ESRGAN's pixel-attention generator (A-ESRGAN/model.py:87-175: RPA, US, Generator_RPA), the checker of
tests/test_rpa_host.py and tests/test_rpa_gpu.py.  Written from the reference's behaviour; tests/golden/rpa.npz pins it to the
reference's own float64 outputs.

    rpa(x, state, ...), us(x, state, ...), generator_rpa(x, state, scale, ...)
Switches, as in tests/attention_oracle.py:
  dtype    torch.float64 (the oracle) or torch.float32 (the same statements in single precision: its gap to the float64 run is the
           yardstick G of the exact-fp32 mode).
  emulate  None, torch.float16 or torch.bfloat16: rounds to that type where the HIP path stores a tensor in it (the list is in
           sr_gan_fd_amd/engine_rpa.py's docstring) and leaves everything else in ``dtype``.  Its gap to the plain float64 run is the
           yardstick E of the 16-bit modes.
  d_out    the incoming gradient; with it the result also holds "dx" and one gradient per parameter under its state-dict key.
  low_res  (us, generator_rpa) True: the HIP path's order -- conv1, LeakyReLU, pa_conv and the gate at the low resolution, then the
           nearest-x2 copy; False: the reference's literal order, up-sampling first.  The two are equal value for value in the forward
           (per-pixel layers commute with replication); the fixture is reproduced in both.
  probe    a dict that receives "pre": every LeakyReLU pre-activation, and "sig": every sigmoid(a), detached (the host tests' margin and
           quantile conditions).
Gradients are torch autograd's over these statements; a rounding point of a stored gradient is an identity whose backward rounds.
"""
import functools
import math

import torch
import torch.nn.functional as F


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


class _Net:
    """the statements shared by the three modules over one dict of parameter leaves"""

    def __init__(self, leaves, emulate, probe):
        self.p, self.em, self.probe = leaves, emulate, probe

    def note(self, key, t):
        if self.probe is not None:
            self.probe.setdefault(key, []).append(t.detach())

    def conv(self, x, name, pad):
        return F.conv2d(x, _r(self.p[name + ".weight"], self.em), self.p[name + ".bias"], padding=pad)

    def lrelu(self, pre):
        """LeakyReLU of a pre-activation whose gradient is stored"""
        self.note("pre", pre)
        return F.leaky_relu(_r(pre, self.em, fwd=False, bwd=True), 0.2)

    def act(self, pre):
        return _r(self.lrelu(pre), self.em)

    def gate(self, x, a):
        """x * sigmoid(a) + x with a, the result and their gradients stored, and the gradient that reaches x directly stored too"""
        a = _r(a, self.em, bwd=True)
        s = torch.sigmoid(a)
        self.note("sig", s)
        return _r(_r(x, self.em, fwd=False, bwd=True) * (1 + s), self.em, bwd=True)

    def rpa(self, x, pre, skip=None):
        h1 = self.act(self.conv(x, pre + "conv1", 0))
        h2 = self.act(self.conv(h1, pre + "conv2", 0))
        g = self.gate(x, self.conv(h2, pre + "conv3", 1))
        y = self.lrelu(self.conv(g, pre + "conv4", 1))
        if skip is None:
            return _r(y, self.em)
        return _r(skip + y, self.em, bwd=True)          # the generator's long skip: one rounding of the sum, its gradient stored

    def us(self, x, pre, low_res=True):
        up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")
        if not low_res:
            x = up(x)
        u = self.act(self.conv(x, pre + "conv1", 0))
        g = self.gate(u, self.conv(u, pre + "pa_conv", 0))
        if low_res:
            g = _r(up(g), self.em, fwd=False, bwd=True)   # conv2's data gradient is stored at the high resolution before the 2x2 sum
        return self.act(self.conv(g, pre + "conv2", 1))


def _run(build, x, state, dtype, emulate, d_out, probe):
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(d_out is not None) for k, v in state.items()}
    xl = x.detach().to(dtype).clone().requires_grad_(d_out is not None)
    out = build(_Net(leaves, emulate, probe), _r(xl, emulate))
    res = {"out": out.detach()}
    if d_out is not None:
        out.backward(_r(d_out.to(dtype), emulate))
        res["dx"] = xl.grad
        for k, v in leaves.items():
            res[k] = v.grad
    return res


def rpa(x, state, dtype=torch.float64, emulate=None, d_out=None, probe=None):
    return _run(lambda net, xi: net.rpa(xi, ""), x, state, dtype, emulate, d_out, probe)


def us(x, state, dtype=torch.float64, emulate=None, d_out=None, probe=None, low_res=True):
    return _run(lambda net, xi: net.us(xi, "", low_res), x, state, dtype, emulate, d_out, probe)


def generator_rpa(x, state, scale, dtype=torch.float64, emulate=None, d_out=None, probe=None, low_res=True):
    num_block = len({k.split(".")[1] for k in state if k.startswith("rpa.")})
    num_us = math.ceil(math.log2(scale))

    def build(net, xi):
        z0 = cur = net.act(net.conv(xi, "conv1", 1))
        for i in range(num_block):
            cur = net.rpa(cur, "rpa.rpa%d." % i, skip=z0 if i == num_block - 1 else None)
        for i in range(num_us):
            cur = net.us(cur, "us.us%d." % i, low_res)
        return net.conv(net.act(net.conv(cur, "conv2", 1)), "conv3", 1)
    return _run(build, x, state, dtype, emulate, d_out, probe)


# ---- inputs ----
def conv_shapes(kind, num_feat, num_block=1, scale=2, num_in_ch=3, num_out_ch=3):
    """(state-dict prefix, cout, cin, ksize) of every conv, in the reference's construction (= state dict) order"""
    f = num_feat
    rpa_ = lambda p: [(p + "conv1", 2 * f, f, 1), (p + "conv2", 4 * f, 2 * f, 1), (p + "conv3", f, 4 * f, 3), (p + "conv4", f, f, 3)]
    us_ = lambda p: [(p + "conv1", f, f, 1), (p + "pa_conv", f, f, 1), (p + "conv2", f, f, 3)]
    if kind == "rpa":
        return rpa_("")
    if kind == "us":
        return us_("")
    out = [("conv1", f, num_in_ch, 3)]
    for i in range(num_block):
        out += rpa_("rpa.rpa%d." % i)
    for i in range(math.ceil(math.log2(scale))):
        out += us_("us.us%d." % i)
    return out + [("conv2", f // 2, f, 3), ("conv3", num_out_ch, f // 2, 3)]


RPA_GATE_SCALE, US_GATE_SCALE = 400.0, 16.0


def make_case(kind, shape, seed, num_feat=64, num_block=1, scale=2):
    """The input recipe of the RPA tests.  x ~ N(0, 1) (an image: uniform in [0, 1)); parameters drawn the way the reference's
    constructors draw theirs (nn.Conv2d's own initialisation; conv1..3 of an RPA normal(0, 2 / fan_in) times 0.1), then each RPA's
    conv3.weight times 400 and each US's pa_conv.weight times 16: with the reference's own scale sigmoid(a) stays within 0.49-0.51,
    the gate is a factor 1.5 and a wrong gate hides below the tolerance.  The incoming gradient ~ N(0, 1) in steps of 1/8.  Every value
    lies on the float16 grid, so a fixture can hold it in that type.  Returns (x, state dict with the module's keys, d_out)."""
    g = torch.Generator().manual_seed(seed)
    grid = lambda t: t.to(torch.float16).to(torch.float32)
    state = {}
    for name, co, ci, k in conv_shapes(kind, num_feat, num_block, scale):
        fan_in = ci * k * k
        leaf = name.rsplit(".", 1)[-1]
        if "rpa" in (kind, name.split(".")[0]) and leaf in ("conv1", "conv2", "conv3"):
            wt = torch.randn(co, ci, k, k, generator=g) * (0.1 * math.sqrt(2.0 / fan_in))
        else:
            wt = (torch.rand(co, ci, k, k, generator=g) * 2 - 1) / math.sqrt(fan_in)
        if "rpa" in (kind, name.split(".")[0]) and leaf == "conv3":
            wt = wt * RPA_GATE_SCALE
        if leaf == "pa_conv":
            wt = wt * US_GATE_SCALE
        state[name + ".weight"] = grid(wt)
        state[name + ".bias"] = grid((torch.rand(co, generator=g) * 2 - 1) / math.sqrt(fan_in))
    x = grid(torch.rand(*shape, generator=g) if kind == "gen" else torch.randn(*shape, generator=g))
    n, _, h, w = shape
    up = 1 if kind == "rpa" else (2 if kind == "us" else 2 ** math.ceil(math.log2(scale)))
    cout = 3 if kind == "gen" else num_feat
    d_out = torch.round(torch.randn(n, cout, h * up, w * up, generator=g) * 8.0) / 8.0
    return x, state, d_out


def run_case(kind, x, state, scale=2, **kw):
    if kind == "rpa":
        return rpa(x, state, **kw)
    if kind == "us":
        return us(x, state, **kw)
    return generator_rpa(x, state, scale, **kw)


# name: (kind, input shape, num_feat, num_block, scale, seed).  The seeds are the first (from 0) at which the oracle alone meets the
# host tests' conditions: the sigmoid quantiles, the LeakyReLU zero margin, and the caps on E (tests/test_rpa_host.py).
CASES = {
    "rpa_5x7": ("rpa", (2, 64, 5, 7), 64, 1, 1, 0),
    "rpa_16x16": ("rpa", (1, 64, 16, 16), 64, 1, 1, 3),
    "us_5x7": ("us", (1, 64, 5, 7), 64, 1, 2, 0),
    "gen2_9x6": ("gen", (1, 3, 9, 6), 64, 2, 2, 1),
    "gen2_5x7": ("gen", (2, 3, 5, 7), 64, 2, 2, 0),
    "gen4_4x6": ("gen", (1, 3, 4, 6), 64, 2, 4, 0),
    "gen1_6x5": ("gen", (1, 3, 6, 5), 64, 1, 1, 0),
}
# the fixture's cases: the reference's classes at num_feat 4 (CPU only: the HIP modules need multiples of 32 / 64)
FIXTURE_CASES = {
    "rpa4": ("rpa", (2, 4, 5, 7), 4, 1, 1, 100),
    "us4": ("us", (1, 4, 5, 7), 4, 1, 2, 101),
    "gen2_4": ("gen", (1, 3, 9, 6), 4, 2, 2, 102),
    "gen4_4": ("gen", (1, 3, 4, 6), 4, 2, 4, 103),
}


def case_inputs(name):
    kind, shape, nf, nb, scale, seed = {**CASES, **FIXTURE_CASES}[name]
    return (kind, scale) + make_case(kind, shape, seed, nf, nb, scale)


@functools.lru_cache(maxsize=None)
def runs(name):
    """inputs and the four oracle runs of one case, computed once and shared by every test that needs them (read-only)"""
    kind, scale, x, state, d_out = case_inputs(name)
    probe = {}
    res = {"kind": kind, "scale": scale, "x": x, "state": state, "d_out": d_out, "probe": probe,
           "f64": run_case(kind, x, state, scale, d_out=d_out, probe=probe),
           "f32": run_case(kind, x, state, scale, d_out=d_out, dtype=torch.float32),
           "f16": run_case(kind, x, state, scale, d_out=d_out, emulate=torch.float16),
           "bf16": run_case(kind, x, state, scale, d_out=d_out, emulate=torch.bfloat16)}
    return res


def max_gap(a, ref):
    """largest absolute difference over the tensor's largest magnitude in the reference"""
    return float((a.double() - ref).abs().max() / ref.abs().max())


def l2_gap(a, ref):
    """relative L2 error"""
    return float((a.double() - ref).norm() / ref.norm())


def sigmoid_quantiles(probe):
    sig = torch.cat([s.flatten() for s in probe["sig"]])
    q = torch.quantile(sig, torch.tensor([0.05, 0.95], dtype=sig.dtype))
    return float(q[0]), float(q[1])


def zero_margin(probe):
    """smallest |pre-activation| of any LeakyReLU, relative to its tensor's largest magnitude"""
    return min(float(p.abs().min() / p.abs().max()) for p in probe["pre"])
