"""Writes tests/golden/niqe.npz: inputs, a synthetic NIQE model and, for each case, what the reference project's torch NIQE
(BSRGAN/image_quality_assessment.py:1138-1333) computes on the CPU -- its rounded luma plane, its half-size plane, its
(N, blocks, 36) feature matrix and its score.  Data only; the intermediates are captured by wrapping the reference's functions at
run time.  Inputs on the u8 grid are stored as uint8 (case C: a 10-bit grid, uint16), images as differences along the width
(delta_x), the half-size plane as the float32 values the reference's resize produces; tests/niqe_oracle.py:load_cases reads it back.

    python tests/golden/make_golden_niqe.py /path/to/reference        (or SRGAN_REFERENCE in the environment)

The published niqe_model.mat is not used: the model is a random mean and a random symmetric positive-definite covariance with
eigenvalues >= 0.1, written with scipy's savemat so that the reference's own loadmat path runs.

Two conditions are enforced on the inputs (the script aborts if one fails), so that any correct implementation reproduces the
integers and table picks exactly:
  * no rounding ties in the luma: every pixel's y*255, recomputed in fp64, lies >= 1e-3 from a half-integer (float32 evaluation
    order moves it by ~1e-5); offending pixels get their G channel nudged by one grid step;
  * no near-ties in the AGGD table search: (second-best - best |r_gam - rhat_norm|) / rhat_norm >= 1e-9 for every block and map
    (fp64 summation-order noise is ~1e-13), and every map of every block has >= 100 negative and >= 100 positive entries.
"""
import importlib
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import niqe_oracle as NO  # noqa: E402

# name: (n, h, w, crop_border, block, grid levels of the stored input)
CASES = {"A": (2, 200, 296, 4, 96, 255), "B": (1, 392, 300, 0, 96, 255), "C": (2, 136, 200, 4, 48, 1023)}
TIE_MARGIN, GAP_MIN, COUNT_MIN = 1e-3, 1e-9, 100


def import_reference(ref):
    if "cv2" not in sys.modules:
        sys.modules["cv2"] = types.ModuleType("cv2")
    path = os.path.join(ref, "BSRGAN")
    sys.path.insert(0, path)
    try:
        for m in ("imgproc", "image_quality_assessment"):
            sys.modules.pop(m, None)
        importlib.import_module("imgproc")
        return importlib.import_module("image_quality_assessment")
    finally:
        sys.path.remove(path)


def make_image(rng, n, h, w, levels):
    """smooth structure plus noise, lightly blurred, clamped to [0,1], on a grid of `levels` steps (integers returned)"""
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    img = np.zeros((n, 3, h, w))
    for i in range(n):
        for c in range(3):
            f = rng.uniform(1.5, 6.0, size=4)
            p = rng.uniform(0, 2 * np.pi, size=4)
            smooth = 0.5 + 0.18 * np.sin(2 * np.pi * f[0] * xx + p[0]) * np.cos(2 * np.pi * f[1] * yy + p[1]) \
                + 0.12 * np.sin(2 * np.pi * (f[2] * xx + f[3] * yy) + p[2]) + 0.1 * (xx - yy) * np.cos(p[3])
            noisy = np.pad(smooth + rng.normal(0, 0.05, size=(h, w)), 1, mode="edge")
            k = np.array([1.0, 2.0, 1.0]) / 4
            blur = sum(k[a] * k[b] * noisy[a:a + h, b:b + w] for a in range(3) for b in range(3))
            img[i, c] = blur
    return np.rint(np.clip(img, 0, 1) * levels).astype(np.int64)


def delta_x(a):
    """differences along the width in the array's own unsigned type (wrapping); np.cumsum(d, axis=-1, dtype=d.dtype) restores the
    array exactly.  The smooth part of the images spreads their values over the whole range, so deflate gains nothing on them as they
    are; their differences are narrow and compress to about half."""
    d = a.copy()
    d[..., 1:] = a[..., 1:] - a[..., :-1]
    assert (np.cumsum(d, axis=-1, dtype=a.dtype) == a).all()
    return d


def remove_luma_ties(q, levels):
    """nudge G where the fp64 luma x255 lies within TIE_MARGIN of a half-integer"""
    for _ in range(50):
        x = q.astype(np.float64) / levels
        y = 65.481 * x[:, 0] + 128.553 * x[:, 1] + 24.966 * x[:, 2] + 16.0
        bad = np.abs(y - np.floor(y) - 0.5) < TIE_MARGIN
        if not bad.any():
            return q
        g = q[:, 1]
        g[bad] += np.where(g[bad] < levels // 2, 1, -1)
    raise SystemExit("luma ties remain")


def check_fits(luma, half, block, tab):
    """the generator's conditions on every AGGD fit; returns (minimum relative gap, minimum sign count)"""
    gap_min, count_min = np.inf, np.inf
    for img in range(luma.shape[0]):
        for plane, b in ((luma[img], block), (half[img] * 255.0, block // 2)):
            s = NO.mscn(plane)
            for by in range(plane.shape[0] // b):
                for bx in range(plane.shape[1] // b):
                    blk = s[by * b:(by + 1) * b, bx * b:(bx + 1) * b]
                    for m in [blk] + [blk * np.roll(blk, sh, axis=(0, 1)) for sh in NO.SHIFTS]:
                        sums = NO.six_sums(m)
                        d, rn = NO.aggd_fit(sums, m.size, tab)[4]
                        two = np.partition(d, 1)[:2]
                        gap_min = min(gap_min, (two[1] - two[0]) / rn)
                        count_min = min(count_min, sums[0], sums[1])
    return gap_min, count_min


def main(ref):
    from scipy.io import savemat
    iqa = import_reference(ref)
    rng = np.random.RandomState(20240607)
    q, _ = np.linalg.qr(rng.normal(size=(36, 36)))
    cov = (q * rng.uniform(0.1, 2.0, size=36)) @ q.T
    cov = (cov + cov.T) / 2
    mu = rng.uniform(0.0, 1.0, size=(1, 36))
    out = {"mu_prisparam": mu, "cov_prisparam": cov}
    tab = NO.aggd_tables()
    assert (np.diff(tab[0]) > 0).all() and (np.diff(tab[1]) > 0).all(), "the shape table must be strictly monotonic"

    captured = {}
    fit, resize, nanmean = iqa._fit_mscn_ipac_torch, iqa._image_resize_torch, iqa._nanmean_torch

    def fit_w(t, *a, **k):
        captured["luma"] = t.clone()
        return fit(t, *a, **k)

    def resize_w(t, *a, **k):
        r = resize(t, *a, **k)
        captured["half"] = r.clone()
        return r

    def nanmean_w(v, *a, **k):
        captured["feat"] = v.clone()
        return nanmean(v, *a, **k)

    iqa._fit_mscn_ipac_torch, iqa._image_resize_torch, iqa._nanmean_torch = fit_w, resize_w, nanmean_w
    conds = []
    with tempfile.TemporaryDirectory() as tmp:
        model = os.path.join(tmp, "niqe_model.mat")
        savemat(model, {"mu_prisparam": mu, "cov_prisparam": cov})
        for name, (n, h, w, cb, block, levels) in CASES.items():
            qimg = remove_luma_ties(make_image(rng, n, h, w, levels), levels)
            stored = qimg.astype(np.uint8 if levels == 255 else np.uint16)
            x = torch.from_numpy(stored.astype(np.float32) / np.float32(levels))      # the expression the tests repeat
            score = iqa.NIQE(cb, model, block, block)(x).reshape(n).to(torch.float64).numpy()
            luma = captured["luma"][:, 0].numpy()
            luma = luma[:, :luma.shape[1] // block * block, :luma.shape[2] // block * block]
            half, feat = captured["half"][:, 0].numpy(), captured["feat"].numpy()
            assert luma.dtype == half.dtype == feat.dtype == np.float64 and (luma == np.rint(luma)).all()
            assert feat.shape == (n, (luma.shape[1] // block) * (luma.shape[2] // block), 36) and feat.shape[1] >= 6
            assert not np.isnan(feat).any()
            half32 = half.astype(np.float32)          # the reference's resize runs in float32: nothing is lost
            assert (half32.astype(np.float64) == half).all()
            gap, cnt = check_fits(luma, half, block, tab)
            print(f"case {name}: scores {score}, min table gap {gap:.2e}, min sign count {cnt:.0f}")
            if gap < GAP_MIN or cnt < COUNT_MIN:
                raise SystemExit(f"case {name}: near-tie in the table search or too few signed entries")
            for i in range(n):
                d = feat[i] - feat[i].mean(0)
                cov_p = cov.astype(np.float32).astype(np.float64)
                conds.append(np.linalg.cond((cov_p + d.T @ d / (feat.shape[1] - 1)) / 2))
            out.update({f"{name}_input_dx": delta_x(stored), f"{name}_params": np.array([cb, block, levels]),
                        f"{name}_luma_dx": delta_x(luma.astype(np.uint8)), f"{name}_half": half32, f"{name}_feat": feat, f"{name}_score": score})
    out["cond_max"] = np.array(max(conds))
    print("condition number of the averaged covariance, maximum:", out["cond_max"])
    path = os.path.join(HERE, "niqe.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ["SRGAN_REFERENCE"])
