"""Float64 statements of what every training step ends in: csrc/elementwise.hip's maps (LeakyReLU backward from act - skip, axpby,
sigmoid and its backward), csrc/loss.hip's losses, their gradients, the non-finite flag and the loss scaler, and csrc/optim.hip's
Adam + EMA step.  The checker of tests/test_step_host.py (which pins every function here to torch's own float64 operators, to
torch.optim.Adam, AveragedModel and torch._amp_update_scale_), tests/test_elementwise_gpu.py, tests/test_loss_gpu.py and
tests/test_optim_gpu.py.

The conventions, bounds and the channel-slice ``Slot`` are those of tests/norm_oracle.py: inputs in the type the kernel sees, widened
here; every function works on whatever device its inputs are on, so that a large case can compute its reference on the GPU.
"""
import numpy as np
import torch

from tests.norm_oracle import (f64, Slot, assert_stored, assert_f32, ulp, bits, abi, code,      # noqa: F401
                               SENTINEL, TOL_FWD, TOL_BWD, F64)
from tests.resample_oracle import assert_bits      # noqa: F401

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]
FLT_MAX = 3.4028234663852886e38
# fp32 values a kernel may treat specially: both zeros, NaN, both infinities, the largest finite number with either sign, the smallest
# subnormal and the smallest normal number (the style of resample_oracle.SPECIAL)
SPECIAL = [0.0, -0.0, float("nan"), float("inf"), -float("inf"), FLT_MAX, -FLT_MAX, 2.0 ** -149, -2.0 ** -126, 1.0, -2.5]
SPECIAL_FINITE = [True, True, False, False, False, True, True, True, True, True, True]


def vn(dtype):
    return 4 if dtype == torch.float32 else 8                # channels per 16-byte vector


def f32(x):
    """a Python number as the kernel receives it: rounded to fp32"""
    return float(np.float32(x))


# ---- elementwise maps ----
def lrelu_backward(dy, act, skip=None, slope=0.2):
    """dy * (act - skip > 0 ? 1 : slope): 0, -0 and NaN count as the slope side (ATen's leaky_relu_backward, `self > 0`).  The
    difference is taken here in float64, where it is exact for 16-bit inputs: its sign is the sign of the fp32 difference."""
    dy, z = f64(dy), f64(act)
    if skip is not None:
        z = z - f64(skip)
    return torch.where(z > 0, dy, dy * float(slope))


def axpby(x, y, alpha, beta):
    """alpha * x + beta * y; beta == 0 does not read y"""
    x = f64(x)
    return alpha * x + (beta * f64(y) if beta != 0 else torch.zeros_like(x))


def sigmoid(x):
    """1 / (1 + exp(-x)), written so that neither side overflows"""
    x = f64(x)
    e = torch.exp(-x.abs())
    return torch.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def sigmoid_backward(ds, s):
    """ds * s * (1 - s) from the stored sigmoid s"""
    ds, s = f64(ds), f64(s)
    return ds * s * (1.0 - s)


def sign(d):
    """torch.sign, (0 < d) - (d < 0): 0 at either zero and at a NaN"""
    return (d > 0).to(d.dtype) - (d < 0).to(d.dtype)


def relu(x):
    """torch.relu: a NaN stays one"""
    return torch.where(x < 0, torch.zeros_like(x), x)


# ---- losses: (loss, gradients of the loss) ----
def l1(a, b, weight=1.0):
    """weight * mean |a - b| -> (loss, d loss / d a = weight * sign(a - b) / n)"""
    d = f64(a) - f64(b)
    return weight * d.abs().mean(), weight * sign(d) / d.numel()


def l1_views(a, b, relu_first=False):
    """mean |a - b| over everything, after torch.relu of both where asked"""
    a, b = f64(a), f64(b)
    if relu_first:
        a, b = relu(a), relu(b)
    return (a - b).abs().mean()


def l1_grad_views(a, b, scale, upstream=None):
    """scale * upstream * sign(a - b)"""
    s = scale * (1.0 if upstream is None else float(upstream))
    return s * sign(f64(a) - f64(b))


def bce_terms(v, target):
    """BCE-with-logits against the constant label, element-wise: max(v, 0) - v * target + log(1 + exp(-|v|))"""
    return torch.clamp(v, min=0.0) - v * target + torch.log1p(torch.exp(-v.abs()))


def bce(x, target):
    """-> (mean BCE-with-logits(x, target), mean sigmoid(x), d loss / d x = (sigmoid(x) - target) / n)"""
    x = f64(x)
    s = sigmoid(x)
    return bce_terms(x, target).mean(), s.mean(), (s - target) / x.numel()


def bce_relativistic(x, other, target):
    """mean_i BCE-with-logits(x_i - mean(other), target) -> (loss, d loss / d x, d loss / d other): other enters through its mean alone,
    so each of its elements gets -sum_i(d loss / d x_i) / n_other"""
    x, other = f64(x), f64(other)
    v = x - other.mean()
    gx = (sigmoid(v) - target) / x.numel()
    return bce_terms(v, target).mean(), gx, torch.full_like(other, -(gx.sum() / other.numel()).item())


def sigmoid_of_mean(x):
    return sigmoid(f64(x).mean())


def nonfinite(x):
    """1.0 if any element is an infinity or a NaN, else 0.0"""
    return 0.0 if bool(torch.isfinite(x).all()) else 1.0


# ---- Adam + EMA, exactly one step ----
def hyper(lr, b1, b2, eps, wd=0.0, ema_decay=0.999):
    """the step's constants as the kernel receives them (fp32)"""
    return dict(lr=f32(lr), b1=f32(b1), b2=f32(b2), eps=f32(eps), wd=f32(wd), ema_decay=f32(ema_decay))


def adam_step(p, g, m, v, ema, hp, t, grad_scale=1.0, ema_mode=0, skipped=False):
    """torch.optim.Adam's step number t (counted from 1) from the given state, weight decay added to the gradient, then the EMA:
    ema_mode 0 none, 1 copy, 2 ema = (1 - decay) * ema + decay * p (the reference's avg_fn).  A skipped step (GradScaler.step on a
    non-finite gradient) leaves p, m, v alone; the EMA still advances from the unchanged p.  -> (p, m, v, ema)"""
    p, m, v = f64(p), f64(m), f64(v)
    if not skipped:
        gi = f64(g) * grad_scale
        if hp["wd"] != 0:
            gi = gi + hp["wd"] * p
        m = hp["b1"] * m + (1.0 - hp["b1"]) * gi
        v = hp["b2"] * v + (1.0 - hp["b2"]) * gi * gi
        bc1, bc2_sqrt = 1.0 - hp["b1"] ** t, (1.0 - hp["b2"] ** t) ** 0.5
        p = p - (hp["lr"] / bc1) * (m / (torch.sqrt(v) / bc2_sqrt + hp["eps"]))
    if ema_mode == 1:
        ema = p.clone()
    elif ema_mode == 2:
        ema = (1.0 - hp["ema_decay"]) * f64(ema) + hp["ema_decay"] * p
    return p, m, v, ema


def bias_corrections(b1, b2, t):
    """the two floats both Adam entry points put in front of the step: (float)(1 - b1^t), (float)sqrt(1 - b2^t), in double first"""
    return np.float32(1.0 - float(b1) ** t), np.float32(np.sqrt(1.0 - float(b2) ** t))


# ---- the loss scaler: torch.amp.GradScaler.update() on the library's 8-word state ----
def scale_state(scale, tracker=0, steps=0, skipped=0):
    """{float scale, float 1 / scale, int32 growth tracker, int32 optimizer steps, int32 skipped steps, 0, 0, 0} as 8 int32 words"""
    st = np.zeros(8, dtype=np.int32)
    st.view(np.float32)[0] = scale
    st.view(np.float32)[1] = np.float32(1.0) / np.float32(scale)
    st[2], st[3], st[4] = tracker, steps, skipped
    return st


def loss_scale_update(state, found_inf, growth, backoff, interval):
    """one update; the scale moves in fp32 as torch's does, so every word is exact.  A growth that would overflow keeps the scale."""
    st = np.array(state, dtype=np.int32)
    f = st.view(np.float32)
    scale, tracker = f[0], int(st[2])
    st[3] += 1
    if found_inf != 0:
        scale, tracker = np.float32(scale * np.float32(backoff)), 0
        st[4] += 1
    else:
        tracker += 1
        if tracker >= interval:
            with np.errstate(over="ignore"):
                grown = np.float32(scale * np.float32(growth))
            if np.isfinite(grown):
                scale = grown
            tracker = 0
    f[0], f[1], st[2] = scale, np.float32(1.0) / np.float32(scale), tracker
    return st


# (start, found_inf per call, growth, backoff, interval)
SCALE_SEQUENCES = [
    (65536.0, [0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0], 2.0, 0.5, 3),                      # growth at the interval, back-off resets the tracker
    # every clean step grows and every product rounds.  The factors are exact in fp32: the library takes them as floats, torch as doubles
    (f32(1000.3), [0, 1, 0, 0, 1, 0], 1.5, 0.75, 1),
    (2.0 ** 127, [0, 0, 0, 0, 1, 0, 0], 2.0, 0.5, 2),                                # a growth that would overflow: the scale is kept, the tracker restarts
    (3.0e38, [0, 0], 1.5, 0.5, 1),
]
SCALE_IDS = ["interval3", "interval1-rounding", "overflow-2^127", "overflow-3e38"]


# ---- what the GPU tests share ----
def ulp32(ref):
    """spacing of fp32 at |ref|"""
    ref = f64(ref).abs()
    _, e = torch.frexp(ref)
    return torch.where(ref > 0, torch.ldexp(torch.ones_like(ref), e - 1 - 23), torch.zeros_like(ref))


class Fenced:
    """a flat fp32 array on the GPU between two fences of ``fence`` sentinels; the front fence keeps the data 16-byte aligned"""

    def __init__(self, data=None, n=None, fence=8, fill=SENTINEL, device="cuda"):
        n = int(data.numel() if data is not None else n)
        self.n, self.fence = n, fence
        self.buf = torch.full((n + 2 * fence,), SENTINEL, dtype=torch.float32, device=device)
        self.val = self.buf[fence:fence + n]
        if data is not None:
            self.val.copy_(data.reshape(-1))
        elif fill != SENTINEL:
            self.val.fill_(fill)
        self.before = self.buf.clone()

    def ptr(self):
        return self.val.data_ptr()

    def assert_fences(self, what):
        f = self.fence
        assert (self.buf[:f] == SENTINEL).all() and (self.buf[f + self.n:] == SENTINEL).all(), f"{what}: written outside the array"

    def assert_untouched(self, what):
        assert torch.equal(bits(self.buf), bits(self.before)), f"{what}: written"
