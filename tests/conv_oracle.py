"""Float64 statement of what csrc/conv_igemm.hip computes -- the formula of include/srganfd.h (srganfd_conv_args) with every argument --
the checker of tests/test_conv_oracle_host.py (which pins it to torch's own float64 operators and to autograd) and of
tests/test_conv_paths_gpu.py.

Conventions of tests/norm_oracle.py: NHWC tensors (..., C); ``x``, ``w``, ``r1``, ``r2`` and ``mask`` are passed in the storage type the
kernel reads (a 16-bit input in its 16-bit type) and widened here, ``bias`` and ``alpha_dev`` are fp32.  What is left between a HIP
result and this one is the fp32 accumulation of K = ksize^2 * cin products and ONE rounding of the stored value: ``bound`` states both.

    v    = alpha * alpha_dev * conv(x)[c] + bias[c]
    v    = act(v)                                      none | LeakyReLU(slope) | ReLU
    y2   = post_scale * v                              (the second output: BEFORE the residual adds)
    v    = post_scale * v + r1_scale * r1[c] + r2_scale * r2[c]
    v   *= (mask[c] > 0 ? 1 : mask_slope)
    y[c] = v                                           for c < cout_store
"""
import torch
import torch.nn.functional as F

from tests.norm_oracle import f64, bits, SENTINEL, F64      # noqa: F401

ACT_NONE, ACT_LRELU, ACT_RELU = 0, 1, 2


# ---- logical weights: (cout, cin, k, k) as F.conv2d reads them, for every orientation the packer (csrc/pack.hip) produces ----
def weight_dgrad(wt):
    """pack code 1: the data gradient of a stride-1 conv with weight ``wt`` (co, ci, k, k) is the conv of dy with the channel-swapped,
    tap-flipped weight (ci, co, k, k)"""
    return wt.transpose(0, 1).flip(2, 3).contiguous()


# forms of a stride-2 conv whose data gradient runs as four output-parity classes: (source kernel, source pad, class taps, first pack
# code, class_pad_step, class (0,0)'s pad)
CLASS_FORMS = {"k4s2": (4, 1, 2, 2, 1, 1), "k3s2": (3, 1, 2, 6, 0, 0), "k2s2": (2, 0, 1, 10, 0, 0)}


def weight_class(wt, form, par):
    """the operand of output-parity class par = 2 py + px (pack codes 2.., 6.., 10..): wt (co, ci, K, K) of a stride-2 conv -> the
    (ci, co, kc, kc) weight of the stride-1 conv over dy that yields the gradient's pixels (2 i + py, 2 j + px).  Per axis, class tap a
    takes source tap: 4x4 pad 1 -- parity 0: 3 - 2a, parity 1: 2 - 2a; 3x3 pad 1 -- parity 0: (1, none), parity 1: (2, 0); 2x2 -- the
    one tap = the parity."""
    py, px = par >> 1, par & 1
    taps = {"k4s2": lambda p: [2, 0] if p else [3, 1], "k3s2": lambda p: [2, 0] if p else [1, -1], "k2s2": lambda p: [p]}[form]
    ty, tx = taps(py), taps(px)
    co, ci = wt.shape[:2]
    out = torch.zeros(ci, co, len(ty), len(tx), dtype=wt.dtype)
    for a, sy in enumerate(ty):
        for b, sx in enumerate(tx):
            if sy >= 0 and sx >= 0:
                out[:, :, a, b] = wt[:, :, sy, sx].t()
    return out


def class_pads(form, par):
    """(pad_y, pad_x) of the single-class launch of class ``par``: class (0,0)'s pad minus parity * class_pad_step"""
    _, _, _, _, step, base = CLASS_FORMS[form]
    return base - (par >> 1) * step, base - (par & 1) * step


# ---- the formula ----
def _window_conv(x, w, stride, pad_y, pad_x, h_out, w_out):
    """x (n, h, w, ci) f64, w (co, ci, k, k) f64 -> (n, h_out, w_out, co): output pixel (oy, ox) reads the k x k window that starts at
    (oy * stride - pad_y, ox * stride - pad_x); everything outside x is zero, on all four sides and as far as the outputs reach"""
    k = w.shape[-1]
    h, wd = x.shape[1], x.shape[2]
    need_h, need_w = (h_out - 1) * stride + k, (w_out - 1) * stride + k
    lo_y, lo_x = pad_y, pad_x
    hi_y, hi_x = need_h - h - pad_y, need_w - wd - pad_x
    xp = F.pad(x.permute(0, 3, 1, 2), (max(lo_x, 0), max(hi_x, 0), max(lo_y, 0), max(hi_y, 0)))
    y0, x0 = max(-lo_y, 0), max(-lo_x, 0)                   # a negative pad: the window starts inside the image
    xp = xp[:, :, y0:y0 + need_h, x0:x0 + need_w]
    return F.conv2d(xp, w, None, stride=stride).permute(0, 2, 3, 1)


def conv2d(x, w, *, stride=1, pad=1, up=0, alpha=1.0, alpha_dev=None, bias=None, act=ACT_NONE, slope=0.2, post_scale=1.0,
           r1=None, r1_scale=0.0, r2=None, r2_scale=0.0, mask=None, mask_slope=0.2, cout_store=None, out=None):
    """x (n, h, w, cin), w (cout, cin, k, k) in F.conv2d's orientation -> (y, y2, A), each (n, h_out, w_out, cout_store) float64.
    ``up``: the logical input is the nearest-x2 upsampling of x.  ``out`` = None: the dense output of ksize / stride / pad.  Else one
    output-parity class, a dict(h_out, w_out, sy, sx, oy, ox, pad_y, pad_x): result pixel (i, j) belongs at (i * sy + oy, j * sx + ox)
    of the full image, pad_y / pad_x replace ``pad``, and r1 / r2 / mask are FULL images read at that address; the returned tensors
    hold the class's own pixels.
    A is the same formula on absolute values with the activation and the mask taken as factor 1: the magnitude the fp32 accumulation
    error scales with."""
    x, w = f64(x), f64(w)
    k = w.shape[-1]
    if up:
        x = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    if out is None:
        ho, wo = (x.shape[1] + 2 * pad - k) // stride + 1, (x.shape[2] + 2 * pad - k) // stride + 1
        pad_y = pad_x = pad
        pick = lambda t: f64(t)
    else:
        ho, wo, pad_y, pad_x = out["h_out"], out["w_out"], out["pad_y"], out["pad_x"]
        pick = lambda t: f64(t)[:, out["oy"]::out["sy"], out["ox"]::out["sx"]][:, :ho, :wo]
    cs = w.shape[0] if cout_store is None else cout_store
    w = w[:cs]
    a = float(alpha) * (float(f64(alpha_dev).reshape(-1)[0]) if alpha_dev is not None else 1.0)
    v = a * _window_conv(x, w, stride, pad_y, pad_x, ho, wo)
    A = abs(a) * _window_conv(x.abs(), w.abs(), stride, pad_y, pad_x, ho, wo)
    if bias is not None:
        v = v + f64(bias)[:cs]
        A = A + f64(bias)[:cs].abs()
    if act == ACT_LRELU:
        v = torch.where(v > 0, v, v * float(slope))
    elif act == ACT_RELU:
        v = torch.where(v > 0, v, torch.zeros_like(v))
    v = float(post_scale) * v
    A = abs(float(post_scale)) * A
    y2 = v
    for r, s in ((r1, r1_scale), (r2, r2_scale)):
        if r is not None:
            v = v + float(s) * pick(r)[..., :cs]
            A = A + abs(float(s)) * pick(r)[..., :cs].abs()
    if mask is not None:
        v = torch.where(pick(mask)[..., :cs] > 0, v, v * float(mask_slope))
    return v, y2, A


def conv2d_classes(x, ws, form, **kw):
    """all four output-parity classes of a stride-2 data gradient (srganfd_conv_args.out_classes = 4, or four single-class launches):
    x = dy (n, hd, wd, co), ws = the four class weights -> (y, y2, A) over the full (n, 2 hd, 2 wd, ci) image"""
    n, hd, wd, _ = x.shape
    full = [torch.zeros(n, 2 * hd, 2 * wd, ws[0].shape[0], dtype=F64) for _ in range(3)]
    for par in range(4):
        res = conv2d(x, ws[par], stride=1, out=class_out(form, par, hd, wd), **kw)
        for dst, src in zip(full, res):
            dst[:, (par >> 1)::2, (par & 1)::2] = src
    return tuple(full)


def class_out(form, par, hd, wd):
    pad_y, pad_x = class_pads(form, par)
    return dict(h_out=hd, w_out=wd, sy=2, sx=2, oy=par >> 1, ox=par & 1, pad_y=pad_y, pad_x=pad_x)


# ---- how close a HIP result has to be ----
# round-to-nearest-even of the stored value (csrc/common.hpp rounds once): half a unit of the last place, relative
ROUND_U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
# fp32 accumulation of K products and the epilogue's few operations: the worst case (K + 8) * 2^-24 * A, times 2 because the order in
# which an MFMA sums its 32 (or 2) products is not specified, times 2 for an activation or mask whose sign test flips where |v| is
# below that error
ACC_FACTOR = 4.0
TINY = 2.0 ** -24                       # the smallest f16 subnormal


def bound(ref, A, K, stored):
    """element-wise bound on |got - ref|: u |ref| + ACC_FACTOR (K + 8) 2^-24 A + tiny; ``stored`` = the type the value is stored in"""
    return ROUND_U[stored] * f64(ref).abs() + ACC_FACTOR * (K + 8) * 2.0 ** -24 * f64(A) + TINY


def worst_ratio(got, ref, A, K, stored):
    """(max over elements of |got - ref| / bound, its index): every element counts, <= 1 passes"""
    got, ref = f64(got), f64(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), "result not finite"
    ratio = (got - ref).abs() / bound(ref, A, K, stored)
    i = int(ratio.argmax())
    return float(ratio.reshape(-1)[i]), i


# ---- device buffers ----
def to_planar(t):
    """(n, h, w, C) -> (n, C / 32, h, w, 32): srganfd_view.planar's bytes, every group of 32 channels its own (h, w, 32) plane"""
    n, h, w, c = t.shape
    assert c % 32 == 0
    return t.reshape(n, h, w, c // 32, 32).permute(0, 3, 1, 2, 4).contiguous()


def from_planar(t):
    """(n, C / 32, h, w, 32) -> (n, h, w, C)"""
    n, g, h, w, _ = t.shape
    return t.permute(0, 2, 3, 1, 4).reshape(n, h, w, g * 32).contiguous()


class Buf:
    """An (n, h, w, cbuf) activation buffer in NHWC or planar form and views of channel slices of it.  ``host`` is the logical NHWC
    content in the storage type: garbage (input side: values that would show in the result if read) or the sentinel (output side)
    wherever no data was put.  ``upload`` lays it out on the device, ``download`` reads it back as NHWC."""

    def __init__(self, n, h, w, cbuf, dtype, planar=0, fill="sentinel", gen=None):
        self.planar, self.dtype = int(planar), dtype
        if fill == "sentinel":
            self.host = torch.full((n, h, w, cbuf), SENTINEL, dtype=dtype)
        else:
            self.host = (torch.randn(n, h, w, cbuf, generator=gen) * 3.0).to(dtype)
        self.dev = None

    def put(self, c0, data):
        """data (n, h, w, c) -> channels [c0, c0 + c); returns the stored (rounded) values"""
        self.host[..., c0:c0 + data.shape[-1]] = data.to(self.dtype)
        return self.host[..., c0:c0 + data.shape[-1]]

    def upload(self, device="cuda"):
        self.dev = (to_planar(self.host) if self.planar else self.host.contiguous()).to(device)
        return self

    def view(self, A, c0=0):
        return A.view(self.dev, self.host.shape[-1], c0, self.planar)

    def download(self):
        t = self.dev.cpu()
        return from_planar(t) if self.planar else t

    def assert_outside_untouched(self, got, c0, c, what, pixels=None):
        """``got`` = download(): everything but channels [c0, c0 + c) -- and, with ``pixels`` = (oy, sy, ox, sx), but that class's pixels
        -- still holds what was uploaded, bit for bit"""
        a, b = bits(got).clone(), bits(self.host).clone()
        if pixels is None:
            a[..., c0:c0 + c] = 0
            b[..., c0:c0 + c] = 0
        else:
            oy, sy, ox, sx = pixels
            a[:, oy::sy, ox::sx, c0:c0 + c] = 0
            b[:, oy::sy, ox::sx, c0:c0 + c] = 0
        assert torch.equal(a, b), f"{what}: written outside the view"
