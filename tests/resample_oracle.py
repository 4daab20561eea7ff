"""Float64 statements of what csrc/resample.hip's x2 kernels (bilinear x2 and its adjoint with the fused LeakyReLU', the adjoint of
nearest x2, 2x2 max-pool, the ReLU copy) and csrc/layout.hip's boundary conversions compute: the checker of tests/test_resample_host.py
(which pins every function here to torch's own float64 operators), tests/test_resample_gpu.py and tests/test_layout_gpu.py.

The conventions, bounds and the channel-slice ``Slot`` are those of tests/norm_oracle.py: NHWC tensors (..., C), inputs in the type
the kernel sees, widened here.
"""
import torch

from tests import norm_oracle as _N
from tests.norm_oracle import (f64, resize_matrix, Slot, assert_stored, assert_f32, bits, ulp, abi, code,      # noqa: F401
                               SENTINEL, TOL_FWD, TOL_BWD, F64)

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]

# (n, h, w, c) of the bilinear x2 pair and the adjoint of nearest x2 (h, w: the low-resolution side); "vn" = one 16-byte vector of the type.
# Against the row-grid kernels' 4 rows per thread and 256 threads per block: both borders in one pixel; two rows, one column; a count of
# channel vectors that is no power of two (24 channels: 6 or 3); a partly filled last row group; two column blocks (40 x 8 or 16 > 256)
X2_SHAPES = [(2, 1, 1, "vn"), (2, 2, 1, 8), (2, 3, 2, 24), (2, 5, 13, 64), (1, 9, 40, 64)]
X2_IDS = ["2x1x1xvn", "2x2x1x8", "2x3x2x24", "2x5x13x64", "1x9x40x64"]
# the boundary conversions: a ragged pixel count, two images
LAYOUT_N, LAYOUT_H, LAYOUT_W = 2, 37, 29


# around and at the ends of [0, 1]: exactly 0, exactly 1, -0, NaN, both infinities, one fp32 step above 1, one fp32 step below 0 (the
# smallest subnormal) and the smallest normal number below 0, values well inside and outside, one fp32 step below 1
SPECIAL = [0.0, 1.0, -0.0, float("nan"), float("inf"), -float("inf"), 1.0 + 2.0 ** -23, -2.0 ** -149, -2.0 ** -126, 0.5, -0.25, 1.75, 1.0 - 2.0 ** -24]
SPECIAL_INSIDE = [True, True, True, False, False, False, False, False, False, True, False, False, True]


def vn(dtype):
    return 4 if dtype == torch.float32 else 8                # channels per 16-byte vector


def x2_shape(shape, dtype):
    n, h, w, c = shape
    return n, h, w, (vn(dtype) if c == "vn" else c)


# ---- bilinear x2, align_corners=False ----
def _up2_axis(x, dim):
    """one axis of the forward pass in closed form: out[2k] = .25 x[k-1] + .75 x[k], out[2k+1] = .75 x[k] + .25 x[k+1], the index clamped
    to the axis -- the rows of resize_matrix(n, 2n), without the matrix (an axis of 65536 would need 64 GiB of it)"""
    x = x.movedim(dim, 0)
    xp = torch.cat([x[:1], x, x[-1:]])
    even, odd = 0.25 * xp[:-2] + 0.75 * xp[1:-1], 0.75 * xp[1:-1] + 0.25 * xp[2:]
    return torch.stack([even, odd], 1).reshape((2 * x.shape[0],) + tuple(x.shape[1:])).movedim(0, dim)


def _up2_axis_adjoint(dy, dim):
    """the transpose of _up2_axis: x[k] collects .25 out[2k-1] + .75 out[2k] + .75 out[2k+1] + .25 out[2k+2]; the tap an end loses to the
    clamp (.25 out[0], .25 out[2n-1]) comes back to that end"""
    dy = dy.movedim(dim, 0)
    even, odd = dy[0::2], dy[1::2]
    dx = 0.75 * (even + odd)
    dx[:-1] += 0.25 * even[1:]
    dx[1:] += 0.25 * odd[:-1]
    dx[0] += 0.25 * even[0]
    dx[-1] += 0.25 * odd[-1]
    return dx.movedim(0, dim)


def bilinear_up2(x):
    """x (n, h, w, c) -> (n, 2h, 2w, c): per axis the matrix resize_matrix(k, 2k) (tests/test_resample_host.py holds the two together),
    weights .25 / .75 with the clamped tap folded into the edge -- the kernels' bil_taps"""
    return _up2_axis(_up2_axis(f64(x), 1), 2)


def bilinear_up2_backward(dy, act=None, slope=0.0):
    """the adjoint: dy (n, 2h, 2w, c) -> dx (n, h, w, c).  With ``act`` (the LeakyReLU output of the layer that was upsampled) returns
    (dx, dx * (act > 0 ? 1 : slope)): 0 counts as the negative side."""
    dx = _up2_axis_adjoint(_up2_axis_adjoint(f64(dy), 2), 1)
    if act is None:
        return dx
    return dx, torch.where(f64(act) > 0, dx, dx * float(slope))


# ---- nearest x2 ----
def nearest_up2(x):
    return f64(x).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def nearest_up2_backward(dy):
    """dy (n, 2h, 2w, c) -> the 2x2 sums (n, h, w, c)"""
    dy = f64(dy)
    n, h2, w2, c = dy.shape
    return dy.reshape(n, h2 // 2, 2, w2 // 2, 2, c).sum(dim=(2, 4))


# ---- ReLU copy, 2x2 max-pool ----
def relu(x):
    """torch's relu: a NaN stays a NaN, -0 stays -0"""
    x = f64(x)
    return torch.where(x < 0, torch.zeros_like(x), x)


def maxpool2(x):
    """x (n, h, w, c) -> (n, h // 2, w // 2, c): an odd last row or column is left out (floor)"""
    x = f64(x)
    return _N.maxpool2(x[:, :x.shape[1] // 2 * 2, :x.shape[2] // 2 * 2])


# ---- the boundary conversions of layout.hip ----
def nchw_to_nhwc(x, cpad, mean=None, std=None):
    """x (n, c, h, w) fp32 -> (n, h, w, cpad): (x - mean) / std per channel where given, the channels from c on are zero"""
    x = f64(x)
    n, c, h, w = x.shape
    if mean is not None:
        x = (x - f64(mean).view(1, c, 1, 1)) / f64(std).view(1, c, 1, 1)
    out = torch.zeros(n, h, w, cpad, dtype=F64)
    out[..., :c] = x.permute(0, 2, 3, 1)
    return out


def nhwc_to_nchw(x, clamp01):
    """x (n, h, w, c) -> (n, c, h, w), clamped to [0, 1] on request as torch.clamp does it: a NaN stays a NaN, -0 stays -0"""
    x = f64(x).permute(0, 3, 1, 2)
    if clamp01:
        x = torch.where(x < 0, torch.zeros_like(x), torch.where(x > 1, torch.ones_like(x), x))
    return x.contiguous()


def clamp_grad(dsr, pre, cpad):
    """the gradient of clamp(pre, 0, 1): dsr (n, c, h, w) passes where 0 <= pre <= 1, both ends included (a NaN is outside);
    pre (n, h, w, c) -> (n, h, w, cpad) with zeros from channel c on"""
    dsr, pre = f64(dsr).permute(0, 2, 3, 1), f64(pre)
    n, h, w, c = dsr.shape
    out = torch.zeros(n, h, w, cpad, dtype=F64)
    out[..., :c] = torch.where((pre >= 0) & (pre <= 1), dsr, torch.zeros_like(dsr))
    return out


def nhwc_to_nchw_scaled(x, div):
    """x (n, h, w, c) -> (n, c, h, w) with channel k divided by div[k]"""
    return (f64(x) / f64(div)).permute(0, 3, 1, 2).contiguous()


# ---- comparisons ----
def assert_bits(out, want, what):
    """the same bit patterns, except that any NaN stands for any other (a conversion may change a NaN's payload)"""
    assert out.dtype == want.dtype and out.shape == want.shape, f"{what}: {out.dtype} {tuple(out.shape)} against {want.dtype} {tuple(want.shape)}"
    out, want = out.detach().cpu(), want.detach().cpu()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(out), nan), f"{what}: NaNs differ"
    a, b = bits(out).clone(), bits(want).clone()
    a[nan] = 0
    b[nan] = 0
    bad = (a != b).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} elements differ, the first at {bad[0].tolist()}: {out[tuple(bad[0])].item()!r} against {want[tuple(bad[0])].item()!r}"
