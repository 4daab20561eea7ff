"""Float64 statements of what csrc/norm.hip's BatchNorm and the attention-gate kernels (general bilinear resize, relu(a + b), gate
multiply, 2x2 max-pool and its backward through the preceding ReLU) compute, the checker of tests/test_norm_host.py (which pins every
function here to torch's own float64 operators under autograd), tests/test_norm_gpu.py and tests/test_attention_gate_gpu.py.

Everything works on NHWC tensors (..., C) and takes the inputs as the kernel sees them: a 16-bit input is passed in its 16-bit type and
widened here, so the only differences left to a HIP result are fp32 arithmetic and the one rounding of a stored 16-bit output --
``assert_stored`` allows exactly that.
"""
import numpy as np
import torch

F64 = torch.float64


def f64(t):
    return torch.as_tensor(t).detach().to(F64)


# ---- BatchNorm2d (+ LeakyReLU) ----
def bn_forward(x, gamma, beta, running_mean, running_var, momentum, eps, training, slope=1.0):
    """y = LeakyReLU_slope(gamma * (x - mean) / sqrt(var + eps) + beta) per channel (the last axis) over all other axes.
    training: mean and the BIASED variance of x; the running statistics move by ``momentum`` towards the mean and the UNBIASED variance.
    Otherwise mean and var are the running statistics, which stay.  Returns (y, running_mean, running_var, save) with
    save = [mean | invstd | scale | shift] (4c values), scale = gamma * invstd, shift = beta - mean * scale."""
    x, gamma, beta, rm, rv = f64(x), f64(gamma), f64(beta), f64(running_mean), f64(running_var)
    c = x.shape[-1]
    xf = x.reshape(-1, c)
    n = xf.shape[0]
    if training:
        if n < 2:
            raise ValueError("training-mode BatchNorm needs more than one value per channel")
        mean = xf.sum(0) / n
        var = ((xf - mean) ** 2).sum(0) / n
        rm = (1.0 - momentum) * rm + momentum * mean
        rv = (1.0 - momentum) * rv + momentum * var * n / (n - 1.0)
    else:
        mean, var = rm, rv
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * invstd
    shift = beta - mean * scale
    y = x * scale + shift
    y = torch.where(y > 0, y, y * slope)
    return y, rm, rv, torch.cat([mean, invstd, scale, shift])


def bn_backward(x, dy, gamma, save, act=None, slope=1.0, total=None, global_sums=None):
    """Adjoint of the training-mode bn_forward.  act: the output of the LeakyReLU that followed; dy is first scaled by
    (act > 0 ? 1 : slope) -- 0 counts as the negative side, ATen's leaky_relu_backward -- and ``act`` is taken as given, never recomputed.
      dbeta = sum dy, dgamma = sum dy * xhat, dx = gamma * invstd * (dy - dbeta / n - xhat * dgamma / n),   xhat = (x - mean) * invstd.
    One rank's share of a data-parallel batch: ``total`` = the pixel count of the whole batch and ``global_sums`` = (dbeta, dgamma) summed
    over the ranks enter dx; the returned dgamma and dbeta stay this share's sums.  Returns (dx, dgamma, dbeta)."""
    x, dy, gamma, save = f64(x), f64(dy), f64(gamma), f64(save)
    c = x.shape[-1]
    mean, invstd = save[:c], save[c:2 * c]
    if act is not None:
        dy = torch.where(f64(act) > 0, dy, dy * float(slope))
    xhat = (x - mean) * invstd
    dbeta = dy.reshape(-1, c).sum(0)
    dgamma = (dy * xhat).reshape(-1, c).sum(0)
    n = float(total if total is not None else x.numel() // c)
    sb, sg = (dbeta, dgamma) if global_sums is None else (f64(global_sums[0]), f64(global_sums[1]))
    dx = gamma * invstd * (dy - sb / n - xhat * sg / n)
    return dx, dgamma, dbeta


# ---- bilinear resize to an explicit size, align_corners=False ----
def resize_matrix(n_in, n_out):
    """(n_out, n_in) interpolation matrix of one axis.  ATen's source index for align_corners=False and an explicit output size
    (area_pixel_compute_source_index): src = max(n_in / n_out * (d + 0.5) - 0.5, 0); taps floor(src) and the next index, clamped to the
    last one, with weights 1 - frac and frac."""
    m = torch.zeros(n_out, n_in, dtype=F64)
    scale = n_in / n_out
    for d in range(n_out):
        src = max(scale * (d + 0.5) - 0.5, 0.0)
        i0 = min(int(np.floor(src)), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        frac = src - i0
        m[d, i0] += 1.0 - frac
        m[d, i1] += frac
    return m


# (hi, wi) -> (ho, wo): identity, one source pixel, one output pixel, extreme ratios up and down (the widest gather window of the
# backward), non-integer ratios
RESIZE_PAIRS = [((8, 8), (8, 8)), ((1, 1), (5, 7)), ((5, 7), (1, 1)), ((3, 3), (32, 32)), ((32, 32), (3, 3)), ((10, 10), (8, 8)),
                ((6, 10), (16, 24)), ((9, 13), (17, 33))]


def resize_bilinear(x, ho, wo):
    """x (n, hi, wi, c) -> (n, ho, wo, c)"""
    x = f64(x)
    return torch.einsum("yh,xw,nhwc->nyxc", resize_matrix(x.shape[1], ho), resize_matrix(x.shape[2], wo), x)


def resize_bilinear_backward(dy, hi, wi):
    """the adjoint: dy (n, ho, wo, c) -> dx (n, hi, wi, c)"""
    dy = f64(dy)
    return torch.einsum("yh,xw,nyxc->nhwc", resize_matrix(hi, dy.shape[1]), resize_matrix(wi, dy.shape[2]), dy)


# ---- attention gate ----
def add_relu(a, b):
    return torch.clamp(f64(a) + f64(b), min=0.0)


def gate(x, g):
    """y[p, c] = g[p] * x[p, c];  x (..., c), g (...)"""
    return f64(g).unsqueeze(-1) * f64(x)


def gate_backward(x, g, dy):
    """(dx, dgate): dx = g * dy, dgate[p] = sum_c dy[p, c] * x[p, c]"""
    return f64(g).unsqueeze(-1) * f64(dy), (f64(dy) * f64(x)).sum(-1)


# ---- 2x2 max-pool ----
def _windows(x):
    """(n, h, w, c) -> (n, h/2, w/2, c, 4), the window in row-major order"""
    n, h, w, c = x.shape
    return x.reshape(n, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, c, 4)


def maxpool2(x):
    return _windows(f64(x)).max(dim=-1).values


def maxpool2_relu_backward(x, dy):
    """x: a ReLU's output (n, h, w, c), dy: gradient of maxpool2(x).  Gradient with respect to the ReLU's INPUT: each window's dy goes
    to its first maximum in row-major order (ATen's max_pool2d) if that maximum is positive (ReLU'), every other element gets 0."""
    x, dy = f64(x), f64(dy)
    n, h, w, c = x.shape
    win = _windows(x).numpy()
    arg = torch.from_numpy(np.argmax(win, axis=-1))          # numpy: the first occurrence of the maximum
    g = torch.where(torch.from_numpy(win.max(axis=-1)) > 0, dy, torch.zeros_like(dy))
    dwin = torch.zeros(n, h // 2, w // 2, c, 4, dtype=F64).scatter_(-1, arg.unsqueeze(-1), g.unsqueeze(-1))
    return dwin.reshape(n, h // 2, w // 2, c, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(n, h, w, c)


# ---- how close a HIP result has to be ----
TOL_FWD, TOL_BWD = 1e-5, 1e-4        # fp32 arithmetic against float64, relative to max|ref|: the bounds the first direct tests held against torch fp32
MANTISSA = {torch.bfloat16: 7, torch.float16: 10}


def ulp(ref, dtype):
    """spacing of ``dtype`` at |ref|: 2^-m * 2^floor(log2 |ref|), m stored mantissa bits; 0 at 0"""
    ref = f64(ref).abs()
    _, e = torch.frexp(ref)                                   # |ref| = f * 2^e with f in [0.5, 1): floor(log2 |ref|) = e - 1
    u = torch.ldexp(torch.ones_like(ref), e - 1 - MANTISSA[dtype])
    return torch.where(ref > 0, u, torch.zeros_like(ref))


def rel_err(out, ref):
    ref = f64(ref)
    return ((f64(out).to(ref.device) - ref).abs().max() / (ref.abs().max() + 1e-300)).item()


def assert_f32(out, ref, tol, what):
    """an fp32 result against float64, relative to max|ref|"""
    assert out.dtype == torch.float32, what
    assert torch.isfinite(out).all(), f"{what}: not finite"
    e = rel_err(out, ref)
    print(f"{what}: rel err {e:.2e} (bound {tol:.0e})")
    assert e <= tol, f"{what}: {e:.3e} > {tol:.0e}"


def assert_stored(out, ref, tol, what):
    """a stored result in its own type: fp32 as assert_f32; 16-bit element-wise |out - ref| <= ulp(|ref|) + tol * max|ref| -- one rounding
    of a value computed in fp32 and nothing more"""
    if out.dtype == torch.float32:
        return assert_f32(out, ref, tol, what)
    ref = f64(ref)
    got = f64(out).to(ref.device)
    assert torch.isfinite(got).all(), f"{what}: not finite"
    excess = (got - ref).abs() - ulp(ref, out.dtype) - tol * ref.abs().max()
    worst = excess.max().item()
    print(f"{what}: max excess over one {out.dtype} ulp + {tol:.0e} max|ref|: {worst:.2e}")
    assert worst <= 0.0, f"{what}: element {int(excess.argmax())} is {worst:.3e} past its bound"


def bits(t):
    """the tensor's bit pattern as integers (NaN sentinels compare equal to themselves)"""
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


# ---- channel-slice views for the GPU tests ----
SENTINEL = -768.0                        # exact in every dtype, far from any result


def abi():
    """(binding module, library handle, the current stream)"""
    from sr_gan_fd_amd import _abi as A
    return A, A.lib(), A.stream_ptr()


def code(A, dtype):
    return {torch.float32: A.F32, torch.bfloat16: A.BF16, torch.float16: A.F16}[dtype]


class Slot:
    """a (..., c) channel slice at channel c0 of a (..., c + pad) buffer on the GPU; everything not given as data holds the sentinel"""

    def __init__(self, shape, dtype, data=None, pad=0, c0=0, device="cuda"):
        self.c, self.c0 = shape[-1], c0
        self.buf = torch.full(tuple(shape[:-1]) + (self.c + pad,), SENTINEL, dtype=dtype, device=device)
        if data is not None:
            self.val.copy_(data)
        self.before = self.buf.clone()

    @property
    def val(self):
        return self.buf[..., self.c0:self.c0 + self.c]

    def view(self, A):
        """the library's srganfd_view of this slice"""
        return A.view(self.buf, self.buf.shape[-1], self.c0)

    def assert_untouched(self, what):
        assert torch.equal(bits(self.buf), bits(self.before)), f"{what}: written"

    def assert_outside_untouched(self, what):
        a, b = bits(self.buf).clone(), bits(self.before).clone()
        a[..., self.c0:self.c0 + self.c] = 0
        b[..., self.c0:self.c0 + self.c] = 0
        assert torch.equal(a, b), f"{what}: channels outside the view were written"
