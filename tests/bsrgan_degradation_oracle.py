"""BSRGAN's blind degradation (the reference's imgproc.degradation_process, BSRGAN/imgproc.py:492-562, with the blur of :212-225 and the
JPEG of :284-293) restated in numpy on given draws, for the tests: the checker of ``imgproc.degradation_process_bsrgan`` where neither the
reference nor cv2 / scipy exist.  Only what the reference really runs is here (its ops 2, 3, 4 begin with ``continue``).

  blur()          mirror padding, float64 products and sums in a fixed order (rows of the kernel, then columns), one rounding to float32:
                  what scipy's ndimage.convolve gives for a float32 image and a float64 kernel (cross-correlation; the reference's
                  kernels are point-symmetric, so the flip of a convolution changes nothing)
  half_cv2()      float32 restatements of ``cv2.resize`` to exactly half size: INTER_AREA = ((a + b) + c + d) * 0.25 of the 2 x 2 cell,
                  INTER_LINEAR = 0.5 * (0.5 a + 0.5 b) + 0.5 * (0.5 c + 0.5 d) (the products are exact), INTER_CUBIC = the taps -0.09375,
                  0.59375, 0.59375, -0.09375 (a = -0.75) along x then y with border indices clamped, as float32 fused multiply-add chains
                  (one choice: the device kernel's compiler mixes fused and unfused steps, so the two may differ in the last place).
                  cv2 is not installed where these were written: they are what the package defines, not a pinned copy of cv2.
  half_imresize() image_resize(image, 1 / 2, True) through tests/resize_oracle.py (fp64), clipped, rounded to float32
  before_resize() everything up to the final image_resize, as the uint8 image the last JPEG decodes to: exact integers
  degrade()       before_resize() / 255 through resize_oracle.resize: the LR image in fp64; a float32 evaluation of that last step lies within
                  resize_oracle.bound_for() of it

A record of draws is the dict ``imgproc.bsrgan_degradation_draws`` returns; kernels come from the caller (the recorded scipy-built ones, or
``imgproc.bsrgan_blur_kernels``)."""
import json

import numpy as np

from tests import jpeg_oracle as JO
from tests import resize_oracle as RO

F32 = np.float32


def blur(image, kernel, columns_first=False):
    """(C, H, W) float32, (k, k) float64 -> (C, H, W) float32; ``columns_first`` sums the taps in the other order (the float32 result is
    expected not to care: the tests count where it does)"""
    if columns_first:
        return np.ascontiguousarray(blur(np.asarray(image).transpose(0, 2, 1), np.asarray(kernel).T).transpose(0, 2, 1))
    k = kernel.shape[0]
    r = k // 2
    x = np.pad(np.asarray(image, dtype=np.float32).astype(np.float64), ((0, 0), (r, r), (r, r)), mode="reflect")
    h, w = image.shape[-2:]
    acc = np.zeros(image.shape, dtype=np.float64)
    for i in range(k):
        for j in range(k):
            acc += kernel[i, j] * x[:, i:i + h, j:j + w]
    return acc.astype(np.float32)


def trim_kernel(k25, ksize):
    """the ksize x ksize kernel at the centre of its 25 x 25 array"""
    o = (k25.shape[-1] - ksize) // 2
    return k25[o:o + ksize, o:o + ksize]


def _fma(a, b, c):
    """float32 fused multiply-add: the product is exact in float64, the sum is rounded there and then to float32"""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def half_cv2(image, interp):
    """(C, H, W) float32 with even H, W -> (C, H / 2, W / 2) float32; interp: cv2's code, 1 linear, 2 cubic, 3 area"""
    x = np.asarray(image, dtype=np.float32)
    h, w = x.shape[-2:]
    a, b, c, d = x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]
    if interp == 3:
        return (((a + b) + c) + d) * F32(0.25)
    if interp == 1:
        half = F32(0.5)
        return half * (half * a + half * b) + half * (half * c + half * d)
    if interp == 2:
        taps = [F32(-0.09375), F32(0.59375), F32(0.59375), F32(-0.09375)]
        ys = [np.clip(np.arange(h // 2) * 2 - 1 + t, 0, h - 1) for t in range(4)]
        xs = [np.clip(np.arange(w // 2) * 2 - 1 + t, 0, w - 1) for t in range(4)]
        out = np.zeros((x.shape[0], h // 2, w // 2), dtype=np.float32)
        for t in range(4):
            rows = x[:, ys[t], :]
            acc = np.zeros_like(out)
            for u in range(4):
                acc = _fma(taps[u], rows[:, :, xs[u]], acc)
            out = _fma(taps[t], acc, out)
        return out
    raise ValueError(f"interpolation code {interp}")


def half_imresize(image):
    return np.clip(RO.resize(np.asarray(image, dtype=np.float32), 0.5, True), 0.0, 1.0).astype(np.float32)


def half_step(gt, rec):
    """the image after the optional half-size step (clipped), float32"""
    x = np.asarray(gt, dtype=np.float32)
    if rec["half"] == "cv2":
        return np.clip(half_cv2(x, rec["interp"]), F32(0), F32(1))
    if rec["half"] == "imresize":
        return half_imresize(x)
    return x


def before_resize(gt, rec, kernels, start=None):
    """(3, H, W) float32 GT, one record of draws, that image's two (25 x 25, centred) kernels in running order -> (3, h, w) uint8: the image
    that the final JPEG decodes to.  ``start``: continue from this image after the half-size step and not from the oracle's own"""
    x = half_step(gt, rec) if start is None else np.asarray(start, dtype=np.float32)
    nb = 0
    for kind, p in rec["ops"]:
        if kind == "blur":
            x = blur(x, trim_kernel(kernels[nb], p["ksize"]))
            nb += 1
        elif p:
            x = JO.roundtrip(x, p)
    return JO.roundtrip_u8(JO.quantise(x), rec["final_quality"]).transpose(2, 0, 1)


def degrade(gt, rec, kernels, start=None):
    """-> (LR image in fp64, the bound of one float32 evaluation of the final image_resize around it)"""
    u8 = before_resize(gt, rec, kernels, start)
    x = u8.astype(np.float32) / F32(255.)
    scale = 1 / rec["sf"]
    return RO.resize(x, scale, True), RO.bound_for(x.shape[-2], x.shape[-1], scale, True)


def load_fixture(path):
    """tests/golden/bsrgan_degradation.npz (tests/golden/make_golden_bsrgan_degradation.py) -> {"cases": {name: dict}, "jpeg": {(h, w): (inputs u8 (3, 3, h, w), outputs u8 (3, 4, 3, h, w))}}"""
    z = np.load(path)
    cases = {}
    for name in [str(n) for n in z["names"]]:
        draws = json.loads(str(z[name + "_draws"]))
        for r in draws:
            r["ops"] = [tuple(o) for o in r["ops"]]
        gt = z[name + "_gt"]
        cases[name] = {"gt_u8": gt, "gt": gt.astype(np.float32) / np.float32(255), "seed": int(z[name + "_seed"]), "factor": int(z[name + "_factor"]),
                       "draws": draws, "end": z[name + "_end"], "kernels": z[name + "_kernels"], "half": z[name + "_half"], "lr": z[name + "_lr"],
                       "before": [z[f"{name}_before{n}"] for n in range(len(draws))]}
    jpeg = {tuple(int(v) for v in s): (z["jpeg_%dx%d_in" % tuple(s)], z["jpeg_%dx%d_out" % tuple(s)]) for s in z["jpeg_sizes"]}
    return {"cases": cases, "jpeg": jpeg, "qualities": [int(q) for q in z["jpeg_qualities"]]}
