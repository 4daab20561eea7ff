"""MATLAB's imresize (the reference's imgproc.image_resize, ESRGAN/imgproc.py:34-127, 202-288) restated for the tests: the checker of
sr_gan_fd_amd/csrc/imresize.hip on machines where the reference project does not exist, and for shapes too big for the fixture.

  tables()   one side's weights and first source indices, FLOAT32 like the reference's (its output coordinates are float32; tables
             built in fp64 differ from it by up to 3.6e-6 in the result at scales like 0.3 or 3.0).  Every column is kept: the
             reference drops the outermost pair, whose weights are zero.
  resize()   applies them with the symmetric index rule (-1 -> 0, n -> n - 1), rows then columns, ACCUMULATING IN FP64 and keeping the
             intermediate in fp64: the exact result of the float32 tables, up to 1e-16.
  bound()    what one float32 evaluation may differ from that by.  With P taps and S = max row sum of |w|, one float32 pass on values of
             magnitude <= M errs by at most (P + 3) * 2^-24 * S * M whatever the summation order or FMA use (P products, P - 1 sums, the
             stored result, each within 2^-24 relative); the second pass sees M <= S.  For inputs in [0, 1]:
                 B = 2 * (P + 3) * 2^-24 * S^2
             (3.4e-6 at 1/4, 6.0e-6 at 1/8, 1.6e-6 when enlarging).  Two float32 evaluations differ by at most 2 B.

tests/golden/image_resize.npz (tests/golden/make_golden_resize.py) is read back by load_cases()."""
import math

import numpy as np
import torch

EPS32 = 2.0 ** -24


def cubic(x):
    """Keys' kernel, a = -0.5, on a float32 tensor"""
    ax = x.abs()
    ax2, ax3 = ax ** 2, ax ** 3
    near = (1.5 * ax3 - 2.5 * ax2 + 1) * (ax <= 1).to(ax.dtype)
    far = (-0.5 * ax3 + 2.5 * ax2 - 4 * ax + 2) * ((ax > 1) * (ax <= 2)).to(ax.dtype)
    return near + far


def tables(in_length, out_length, scale, antialiasing=True):
    """-> (weights (out, P) float32, first (out,) int64): output i is sum_k weights[i, k] * sample(first[i] + k), 0-based samples"""
    stretch = scale < 1 and antialiasing
    width = 4 / scale if stretch else 4
    taps = math.ceil(width) + 2
    centre = torch.linspace(1, out_length, out_length) / scale + 0.5 * (1 - 1 / scale)         # 1-based, float32
    left = torch.floor(centre - width / 2)
    sample = left[:, None] + torch.linspace(0, taps - 1, taps)[None, :]
    d = centre[:, None] - sample
    w = scale * cubic(d * scale) if stretch else cubic(d)
    w = w / torch.sum(w, 1)[:, None]
    return w.numpy(), left.numpy().astype(np.int64) - 1


def reflect(j, n):
    """MATLAB's symmetric padding on an index array; one reflection (padding no longer than the side)"""
    j = np.where(j < 0, -1 - j, j)
    j = np.where(j >= n, 2 * n - 1 - j, j)
    return np.clip(j, 0, n - 1)       # only samples of weight 0 are ever clipped (asserted in apply_side)


def apply_side(x, w, first, axis):
    """fp64 weighted sums along `axis`; taps added one after the other (elementwise operations only: the same bits on every machine)"""
    x = np.moveaxis(np.asarray(x, dtype=np.float64), axis, 0)
    n = x.shape[0]
    w = np.asarray(w, dtype=np.float64)
    first = np.asarray(first, dtype=np.int64)
    out = np.zeros((w.shape[0],) + x.shape[1:])
    shape = (-1,) + (1,) * (x.ndim - 1)
    for k in range(w.shape[1]):
        j = first + k
        far = (j < -n) | (j >= 2 * n)
        assert not (far & (w[:, k] != 0)).any(), "a sample further out than one reflection carries weight"
        out += w[:, k].reshape(shape) * x[reflect(j, n)]
    return np.moveaxis(out, 0, axis)


def resize(x, scale, antialiasing=True):
    """(..., H, W) array -> (..., ceil(H * scale), ceil(W * scale)) fp64: rows first, then columns"""
    h, w = x.shape[-2:]
    th = tables(h, math.ceil(h * scale), scale, antialiasing)
    tw = tables(w, math.ceil(w * scale), scale, antialiasing)
    return apply_side(apply_side(x, *th, axis=-2), *tw, axis=-1)


def bound(*weight_tables):
    """B of the module docstring from the weight tables of both sides (P: the most taps, S: the largest row sum of |w|)"""
    p = max(t.shape[1] for t in weight_tables)
    s = max(float(np.abs(np.asarray(t, dtype=np.float64)).sum(1).max()) for t in weight_tables)
    return 2 * (p + 3) * EPS32 * s * s


def bound_for(h, w, scale, antialiasing=True):
    return bound(tables(h, math.ceil(h * scale), scale, antialiasing)[0], tables(w, math.ceil(w * scale), scale, antialiasing)[0])


def table_delta(mine, first_mine, theirs, first_theirs):
    """max |w_a - w_b| between two tables of one side whose column 0 may sit at different samples (one of them dropped zero columns):
    both are spread over the samples they address, so a weight that only one of them holds counts in full"""
    lo = int(min(first_mine.min(), first_theirs.min()))
    hi = int(max((first_mine + mine.shape[1]).max(), (first_theirs + theirs.shape[1]).max()))
    dense = np.zeros((2, mine.shape[0], hi - lo))
    for d, (t, f) in zip(dense, ((mine, first_mine), (theirs, first_theirs))):
        for i in range(t.shape[0]):
            d[i, f[i] - lo:f[i] - lo + t.shape[1]] = t[i]
    return float(np.abs(dense[0] - dense[1]).max())


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
CASE_NAMES = ["q128", "q97x131", "h96x120", "t90x75", "e128x96", "x2_33x47", "x4_40x28", "s03_61x83", "s07_50x70", "s07_50x70_plain",
              "q65x66_plain", "x3_31x18_plain", "q7x9", "s09_301x203", "x15_77x64_2d"]


def ordered(a):
    """float32 -> int64 that rises with the value: the distance between two floats in units in the last place is a difference"""
    i = np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def from_ordered(i):
    i = np.asarray(i, dtype=np.int64)
    return np.where(i < 0, (-i) | 0x80000000, i).astype(np.uint32).view(np.float32)


def anchor(x, wh, first_h, ww, first_w):
    """what the fixture's outputs are stored against: the recorded tables applied in fp64 and rounded to float32"""
    return apply_side(apply_side(x, wh, first_h, axis=-2), ww, first_w, axis=-1).astype(np.float32)


def load_cases(path):
    """tests/golden/image_resize.npz -> {name: dict}.  Inputs are stored on the u8 grid as differences along the width; outputs as the
    distance, in float32 units in the last place, from anchor() of the recorded tables (the reference's float32 values restored bit
    for bit; make_golden_resize.py checks the round trip)."""
    z = np.load(path)
    cases = {}
    for name in [str(n) for n in z["names"]]:
        d = z[name + "_input_dx"]
        scale, aa = float(z[name + "_scale"]), bool(z[name + "_antialiasing"])
        x = np.cumsum(d, axis=-1, dtype=d.dtype).astype(np.float32) / np.float32(255)
        sym = [int(v) for v in z[name + "_sym"]]
        c = {"input": x, "scale": scale, "antialiasing": aa, "sym": sym,
             "weights_h": z[name + "_weights_h"], "indices_h": z[name + "_indices_h"].astype(np.int64),
             "weights_w": z[name + "_weights_w"], "indices_w": z[name + "_indices_w"].astype(np.int64)}
        # the reference's indices address its padded copy: sample = index - sym_len_s
        c["first_h"], c["first_w"] = c["indices_h"][:, 0] - sym[0], c["indices_w"][:, 0] - sym[2]
        base = anchor(x, c["weights_h"], c["first_h"], c["weights_w"], c["first_w"])
        c["output"] = from_ordered(ordered(base) + z[name + "_output_ulps"].astype(np.int64)).reshape(base.shape)
        cases[name] = c
    return cases
