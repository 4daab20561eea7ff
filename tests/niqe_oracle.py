"""NIQE restated in numpy fp64, as plain loops over blocks: the specification the HIP kernels of sr_gan_fd_amd/csrc/iqa.hip are
tested against on machines where the reference project does not exist.  tests/test_niqe_host.py checks that this file reproduces
every case of tests/golden/niqe.npz (planes, features, scores recorded from the reference).

Steps (fp64 after the luma, except step 5):
  1. luma: BT.601 in float32, x255, round half to even, crop to whole blocks;
  2. MSCN map with the float32-rounded 7x7 Gaussian (sigma 7/6), replicate padding;
  3. per block five maps (s and s times its circular shift inside the block), six sums per map;
  4. AGGD fit through the 9801-entry shape table;
  5. half-size image: 10-tap antialiased cubic, symmetric padding, rows then columns, in float32 as the reference runs it;
  6. score: Mahalanobis-like distance between the model and the block features' mean / covariance.
"""
import math

import numpy as np
import torch

SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))


def aggd_tables():
    """(4, 9801) fp64: shape values, their r_gam, and the two gamma-function factors the features need.  The shape grid is the
    float32 arange widened to fp64; torch builds it (numpy's float32 arange rounds differently)."""
    a = torch.arange(0.2, 10 + 0.001, 0.001).to(torch.float64)
    l1, l2, l3 = torch.lgamma(1. / a), torch.lgamma(2. / a), torch.lgamma(3. / a)
    r_gam = (2 * l2 - (l1 + l3)).exp()
    return torch.stack([a, r_gam, (l1 - l3).exp().sqrt(), (l2 - l1).exp()]).numpy()


def gaussian_window():
    """7 x 7, sigma 7/6, normalised in fp64, rounded to float32 and widened again."""
    r = np.arange(-3.0, 4.0)
    h = np.exp(-(r[:, None] ** 2 + r[None, :] ** 2) / (2.0 * (7.0 / 6.0) ** 2))
    h[h < np.finfo(np.float64).eps * h.max()] = 0
    return (h / h.sum()).astype(np.float32).astype(np.float64)


def luma_plane(rgb, crop_border, bh, bw):
    """(N,3,H,W) float32 in [0,1] -> (N,h,w) fp64 holding integers; h, w whole multiples of the block."""
    x = np.asarray(rgb, dtype=np.float32)
    if crop_border > 0:
        x = x[:, :, crop_border:-crop_border, crop_border:-crop_border]
    w = np.float32([65.481, 128.553, 24.966])
    y = x[:, 0] * w[0] + x[:, 1] * w[1] + x[:, 2] * w[2]
    y = (y + np.float32(16.0)) / np.float32(255.0)
    y = np.rint(y * np.float32(255.0)).astype(np.float64)
    h, wd = y.shape[1] // bh * bh, y.shape[2] // bw * bw
    return y[:, :h, :wd]


def cubic(x, a=-0.5):
    ax = abs(x)
    if ax <= 1:
        return (a + 2) * ax ** 3 - (a + 3) * ax ** 2 + 1
    if ax <= 2:
        return a * ax ** 3 - 5 * a * ax ** 2 + 8 * a * ax - 4 * a
    return 0.0


def half_taps():
    """The 10 normalised weights of one output sample of the 0.5x antialiased cubic: sample i reads inputs 2i-4 .. 2i+5."""
    w = np.array([cubic((4.5 - k) * 0.5) for k in range(10)])
    return w / w.sum()


def _half_1d(x, axis):
    """float32 in, float32 out: every product and every partial sum rounded to float32, taps added in index order"""
    n = x.shape[axis]
    out_n = (n + 1) // 2
    taps = half_taps().astype(np.float32)
    x = np.moveaxis(x, axis, 0)
    out = np.zeros((out_n,) + x.shape[1:], dtype=np.float32)
    for i in range(out_n):
        for k in range(10):
            j = 2 * i - 4 + k
            j = -1 - j if j < 0 else (2 * n - 1 - j if j >= n else j)     # symmetric: the edge sample is used twice
            out[i] += taps[k] * x[j]
    return np.moveaxis(out, 0, axis)


def half_size(planes):
    """(..., h, w) fp64 -> (..., ceil(h/2), ceil(w/2)) fp64: rows first, then columns.  The arithmetic is FLOAT32: the reference's
    resize casts whatever it is given to float32 (its dtype test `!= float32 or != float64` is always true) and widens the result
    again, and every score depends on those float32 roundings, so they are part of the specification."""
    x = np.asarray(planes, dtype=np.float64).astype(np.float32)
    return _half_1d(_half_1d(x, -2), -1).astype(np.float64)


def mscn(x):
    """(h, w) fp64 -> the mean-subtracted contrast-normalised map."""
    g = gaussian_window()
    h, w = x.shape
    p = np.pad(x, 3, mode="edge")
    mu, m2 = np.zeros_like(x), np.zeros_like(x)
    for i in range(7):
        for j in range(7):
            t = p[i:i + h, j:j + w]
            mu += g[i, j] * t
            m2 += g[i, j] * (t * t)
    sigma = np.sqrt(np.abs(m2 - mu * mu) + 1e-8)
    return (x - mu) / (sigma + 1.0)


def six_sums(m):
    neg, pos = m < 0, m > 0
    sq = m * m
    return (float(neg.sum()), float(pos.sum()), float(sq[neg].sum()), float(sq[pos].sum()), float(np.abs(m).sum()), float(sq.sum()))


def aggd_fit(sums, n, tab):
    """six sums of one map of n entries -> (alpha, left_beta, right_beta, mean factor); also the table-search gap for the generator."""
    cneg, cpos, sneg, spos, sabs, ssq = sums
    with np.errstate(all="ignore"):
        dl = np.float64(np.float32(cneg) + np.float32(1e-8))
        dr = np.float64(np.float32(cpos) + np.float32(1e-8))
        lstd, rstd = np.sqrt(np.float64(sneg) / dl), np.sqrt(np.float64(spos) / dr)
        gh = lstd / rstd
        rhat = (np.float64(sabs) / n) ** 2 / (np.float64(ssq) / n)
        rn = (rhat * (gh ** 3 + 1) * (gh + 1)) / (gh ** 2 + 1) ** 2
        d = np.abs(tab[1] - rn)
    k = 0 if np.isnan(rn) else int(np.argmin(d))
    return tab[0][k], lstd * tab[2][k], rstd * tab[2][k], tab[3][k], (d, rn)


def block_features(s, tab):
    """one block of the MSCN map -> its 18 features"""
    n = s.size
    a, lb, rb, _, _ = aggd_fit(six_sums(s), n, tab)
    f = [a, (lb + rb) / 2]
    for sh in SHIFTS:
        a, lb, rb, cm, _ = aggd_fit(six_sums(s * np.roll(s, sh, axis=(0, 1))), n, tab)
        f += [a, (rb - lb) * cm, lb, rb]
    return f


def features(luma, bh, bw, tab=None):
    """(N,h,w) fp64 luma -> ((N, blocks, 36) features in column-major block order, (N, ceil(h/2), ceil(w/2)) half-size plane in [0,1])"""
    tab = aggd_tables() if tab is None else tab
    n, h, w = luma.shape
    nby, nbx = h // bh, w // bw
    half = half_size(luma / 255.0)
    out = np.zeros((n, nby * nbx, 36))
    for img in range(n):
        for sc, (plane, sbh, sbw) in enumerate(((luma[img], bh, bw), (half[img] * 255.0, bh // 2, bw // 2))):
            s = mscn(plane)
            for bx in range(nbx):
                for by in range(nby):
                    blk = s[by * sbh:(by + 1) * sbh, bx * sbw:(bx + 1) * sbw]
                    out[img, bx * nby + by, 18 * sc:18 * sc + 18] = block_features(blk, tab)
    return out, half


def score(feat, mu_p, cov_p):
    """(N, blocks, 36) features, model mean (36,) and covariance (36,36) (already passed through float32) -> (N,) scores"""
    out = np.zeros(feat.shape[0])
    for i, f in enumerate(feat):
        nan = np.isnan(f)
        mu_d = np.where(nan, 0.0, f).sum(0) / (~nan).sum(0)
        rows = f[~nan.any(1)]
        d = rows - rows.mean(0)
        cov_d = d.T @ d / (rows.shape[0] - 1)
        diff = mu_p - mu_d
        out[i] = math.sqrt(diff @ np.linalg.pinv((cov_p + cov_d) / 2) @ diff)
    return out


def niqe(rgb, crop_border, mu_p, cov_p, bh=96, bw=96):
    luma = luma_plane(rgb, crop_border, bh, bw)
    feat, half = features(luma, bh, bw)
    mu_p = np.ravel(mu_p).astype(np.float32).astype(np.float64)
    cov_p = np.asarray(cov_p).astype(np.float32).astype(np.float64)
    return score(feat, mu_p, cov_p), luma, half, feat


ALPHA_COLUMNS = [0, 2, 6, 10, 14, 18, 20, 24, 28, 32]      # the AGGD shape parameters among the 36 features


def load_cases(path):
    """tests/golden/niqe.npz -> (model mean, model covariance, maximum condition number, {case: dict}).  The images are stored as
    differences along the width in their unsigned type (see make_golden_niqe.py); cumsum in that type restores them exactly."""
    z = np.load(path)
    cases = {}
    for name in "ABC":
        cb, block, levels = (int(v) for v in z[name + "_params"])
        d, ld = z[name + "_input_dx"], z[name + "_luma_dx"]
        cases[name] = {
            "crop_border": cb, "block": block,
            "input": np.cumsum(d, axis=-1, dtype=d.dtype).astype(np.float32) / np.float32(levels),
            "luma": np.cumsum(ld, axis=-1, dtype=ld.dtype).astype(np.float64),
            "half": z[name + "_half"].astype(np.float64),       # float32 values: the reference's resize runs in float32
            "feat": z[name + "_feat"], "score": z[name + "_score"],
        }
    return z["mu_prisparam"], z["cov_prisparam"], float(z["cond_max"]), cases
