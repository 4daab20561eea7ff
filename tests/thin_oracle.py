"""Float64 statement of what csrc/conv_thin.hip computes -- the three entry points of include/srganfd.h (srganfd_thin_args) with every
argument -- the checker of tests/test_thin_oracle_host.py (which pins it to torch's own float64 operators and to autograd) and of
tests/test_thin_paths_gpu.py.

Conventions of tests/conv_oracle.py: NHWC tensors (..., C); ``thin`` (n, h, w, 4: channels >= cs zero), ``big`` and ``mask`` (n, h, w, 64)
are passed in the 16-bit storage type the kernel reads and widened here; ``bias`` is fp32.  ``w`` is the layer's raw (Cout, Cin, 3, 3)
parameter ROUNDED TO THE ELEMENT TYPE by the caller (``W.to(dt)``): the kernels take the unrounded fp32 tensor and round it themselves
while they build their MFMA operands.

    W(b, s, tap)   = w[b][s][tap'] if w_big_is_cout else w[s][b][tap'],  tap' = 8 - tap if flip else tap       b < 64, s < cs
    thin_in        big[p][b]      = act(bias[b] + sum_{tap, s} W(b, s, tap) * thin[p + tap - 1][s])  * (mask[p][b] > 0 ? 1 : mask_slope)
    thin_out       thin_out[p][s] = bias[s] + sum_{tap, b} W(b, s, tap) * big[p + tap - 1][b]                  fp32
    thin_wgrad     D[b][tap][s]   = sum_p big[p][b] * thin[p + tap - 1][s];  dw[b][s][tap] = D if w_big_is_cout else dw[s][b][8 - tap] = D
                   db[b] = sum_p big[p][b] if w_big_is_cout else db[s] = sum_p thin[p][s]                      fp32

How close a HIP result has to be, per element, is conv_oracle.bound(ref, A, K, stored):
    thin_in              K = 9 cs, stored = the 16-bit type.  With a mask the rounding term is 2 u |ref| instead of u |ref|, which follows
                         from the code and not from a measurement: the value is rounded once into the wave's LDS image, read back,
                         multiplied by (mask > 0 ? 1 : mask_slope) in fp32 and rounded again for the store.
    thin_out             K = 9 * 64, stored = fp32
    thin_wgrad           K = n h w, the length of the fp32 pixel sum; stored = fp32; A = the same sum over absolute values
"""
import torch

from tests import conv_oracle as O
from tests.conv_oracle import f64, F64, ACT_NONE, ACT_LRELU, ACT_RELU      # noqa: F401


def logical_weight(w, w_big_is_cout, flip, thin_is_cin):
    """w (Cout, Cin, 3, 3) -> the (cout, cin, 3, 3) weight F.conv2d needs for a launch whose input is the thin side (thin_is_cin) or
    the 64-channel side: W(b, s, tap) of the module docstring, put as [b][s] resp. [s][b]"""
    big_first = w if w_big_is_cout else w.transpose(0, 1)          # [b][s][tap']
    lw = big_first if thin_is_cin else big_first.transpose(0, 1)
    return (lw.flip(2, 3) if flip else lw).contiguous()


def thin_in(thin, w, cs, *, w_big_is_cout, flip=False, bias=None, act=ACT_NONE, slope=0.2, mask=None, mask_slope=0.2):
    """-> (y, A) float64 (n, h, w, 64); A as in conv_oracle.conv2d"""
    y, _, A = O.conv2d(thin[..., :cs], logical_weight(w, w_big_is_cout, flip, True), bias=bias, act=act, slope=slope, mask=mask, mask_slope=mask_slope)
    return y, A


def thin_out(big, w, cs, *, w_big_is_cout, flip=False, bias=None):
    """-> (y, A) float64 (n, h, w, cs)"""
    y, _, A = O.conv2d(big, logical_weight(w, w_big_is_cout, flip, False), bias=bias)
    return y, A


def thin_wgrad(big, thin, cs, *, w_big_is_cout):
    """-> (dw, db, A_dw, A_db): dw in the raw layout of the conv's weight -- (64, cs, 3, 3) if w_big_is_cout else (cs, 64, 3, 3) -- db its
    bias gradient (64 resp. cs values), the A's the same sums over absolute values"""
    big, thin = f64(big), f64(thin)[..., :cs]
    n, h, w, _ = big.shape

    def sums(bg, tn):
        pad = torch.nn.functional.pad(tn, (0, 0, 1, 1, 1, 1))                   # thin[p + tap - 1] with zeros outside the image
        d = torch.stack([torch.einsum("nhwb,nhws->bs", bg, pad[:, ky:ky + h, kx:kx + w]) for ky in range(3) for kx in range(3)], dim=2)   # [b][s][tap]
        if w_big_is_cout:
            return d.reshape(64, cs, 3, 3), bg.sum(dim=(0, 1, 2))
        return d.flip(2).permute(1, 0, 2).reshape(cs, 64, 3, 3).contiguous(), tn.sum(dim=(0, 1, 2))

    dw, db = sums(big, thin)
    A_dw, A_db = sums(big.abs(), thin.abs())
    return dw, db, A_dw, A_db


def bound_in(ref, A, cs, stored, masked):
    """thin_in's element-wise bound: conv_oracle.bound with K = 9 cs, plus a second rounding of the stored value behind a mask"""
    b = O.bound(ref, A, 9 * cs, stored)
    return b + O.ROUND_U[stored] * f64(ref).abs() if masked else b


def ratio_in(got, ref, A, cs, stored, masked):
    """(max |got - ref| / bound_in, its index): <= 1 passes"""
    got = f64(got)
    assert got.shape == ref.shape and torch.isfinite(got).all()
    r = (got - ref).abs() / bound_in(ref, A, cs, stored, masked)
    i = int(r.argmax())
    return float(r.reshape(-1)[i]), i
