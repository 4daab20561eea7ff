"""Writes tests/golden/bsrgan_degradation.npz: what the reference project's blind degradation (BSRGAN/imgproc.py:492-562
``degradation_process`` with ``_add_blur`` :212-225 and ``_add_jpeg_compression`` :284-293) computes on the CPU for seeded inputs.  Data only.

    python tests/golden/make_golden_bsrgan_degradation.py /path/to/reference        (or SRGAN_REFERENCE in the environment)

Needs scipy and Pillow.  The reference imports cv2, which is not a dependency here; this script installs a stand-in of its own for the four
calls the function makes: ``imencode`` / ``imdecode`` go through Pillow (libjpeg-turbo with default settings, as cv2's do), ``cvtColor`` swaps
the channel order, and ``resize`` is the float32 restatement of tests/bsrgan_degradation_oracle.half_cv2 -- so parity with cv2's JPEG is pinned
only through "both are libjpeg with default settings", and parity with cv2.resize is not pinned at all.  ``scipy.finfo``, which the reference
still calls, is set to ``np.finfo``.

Recorded per degradation case (a small batch degraded image by image after ``random.seed(s)`` / ``np.random.seed(s)``, as the reference's
loader would): the GT batch as uint8 (x = u8.astype(float32) / float32(255), the expression the tests repeat), the seed, the draws as the
package's ``bsrgan_degradation_draws`` returns them after the same seeding (JSON), the next draw of either stream after the batch (the end
state), the scipy-built kernels the reference convolved with (captured at the call, centred in 25 x 25), the image after the half-size step
where one was taken, the uint8 image the final JPEG decoded to, and the LR image.  Per JPEG case: uint8 inputs and their round trips at
q = 30, 47, 50, 95 through Pillow."""
import importlib
import io
import json
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import bsrgan_degradation_oracle as BO  # noqa: E402
from tests import jpeg_oracle as JO  # noqa: E402

SIZE_LIMIT = 512 * 1024
JPEG_SIZES = [(16, 16), (9, 23), (17, 33), (37, 52)]
JPEG_QUALITIES = [30, 47, 50, 95]
KMAX = 25
# name: (factor, batch, (H, W), wanted half-step kinds); the seed is the first one whose draws cover the wanted kinds
CASES = {"x2_32x48": (2, 2, (32, 48), {None}), "x4_64x64": (4, 4, (64, 64), {None, "imresize", "cv2"})}


def cv2_stand_in():
    from PIL import Image
    m = types.ModuleType("cv2")
    m.COLOR_RGB2BGR, m.COLOR_BGR2RGB, m.IMWRITE_JPEG_QUALITY = 4, 4, 1

    def resize(image, dsize, interpolation):
        h, w = image.shape[:2]
        assert dsize == (w // 2, h // 2) and image.dtype == np.float32
        return np.ascontiguousarray(BO.half_cv2(image.transpose(2, 0, 1), interpolation).transpose(1, 2, 0))

    def imencode(ext, image, params):
        assert ext == ".jpg" and image.dtype == np.uint8 and params[0] == m.IMWRITE_JPEG_QUALITY
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(image[..., ::-1])).save(buf, format="JPEG", quality=params[1])
        return True, np.frombuffer(buf.getvalue(), dtype=np.uint8)

    def imdecode(buf, flags):
        return np.ascontiguousarray(np.array(Image.open(io.BytesIO(buf.tobytes())).convert("RGB"))[..., ::-1])

    m.resize, m.imencode, m.imdecode, m.cvtColor = resize, imencode, imdecode, lambda image, code: np.ascontiguousarray(image[..., ::-1])
    return m


def import_reference(ref):
    import scipy
    scipy.finfo = np.finfo
    sys.modules["cv2"] = cv2_stand_in()
    path = os.path.join(ref, "BSRGAN")
    sys.path.insert(0, path)
    try:
        sys.modules.pop("imgproc", None)
        return importlib.import_module("imgproc")
    finally:
        sys.path.remove(path)


def make_image(rng, shape):
    """smooth structure plus noise on the u8 grid, (C, H, W)"""
    h, w = shape[-2:]
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    planes = []
    for _ in range(shape[0]):
        f, p = rng.uniform(0.5, 4.0, size=3), rng.uniform(0, 2 * np.pi, size=3)
        img = 0.5 + 0.25 * np.sin(2 * np.pi * f[0] * xx + p[0]) * np.cos(2 * np.pi * f[1] * yy + p[1]) + 0.2 * np.sin(2 * np.pi * f[2] * (xx + yy) + p[2])
        planes.append(img + rng.normal(0, 0.04, size=(h, w)))
    return np.rint(np.clip(np.stack(planes), 0, 1) * 255).astype(np.uint8)


def seed_all(s):
    random.seed(s)
    np.random.seed(s)


def find_seed(package, factor, batch, kinds):
    for s in range(100000):
        seed_all(s)
        draws = package.bsrgan_degradation_draws(batch, factor)
        if {r["half"] for r in draws} == kinds:
            return s, draws
    raise RuntimeError("no seed covers " + repr(kinds))


def main(ref):
    from scipy import ndimage
    from PIL import Image
    from sr_gan_fd_amd import imgproc as package
    imgproc = import_reference(ref)
    captured = {"kernels": [], "resize": []}

    def convolve(image, weights, mode):
        assert mode == "mirror" and image.dtype == np.float32 and weights.dtype == np.float64
        captured["kernels"].append(weights[:, :, 0].copy())
        return ndimage.convolve(image, weights, mode=mode)

    imgproc.ndimage = types.SimpleNamespace(filters=types.SimpleNamespace(convolve=convolve))
    image_resize = imgproc.image_resize

    def image_resize_w(image, scale, antialiasing=True):
        y = image_resize(image, scale, antialiasing)
        captured["resize"].append((np.array(image, dtype=np.float32).transpose(2, 0, 1), np.array(y, dtype=np.float32).transpose(2, 0, 1)))
        return y

    imgproc.image_resize = image_resize_w
    rng = np.random.RandomState(20250301)
    out = {"names": np.array(list(CASES)), "jpeg_sizes": np.array(JPEG_SIZES), "jpeg_qualities": np.array(JPEG_QUALITIES)}
    for name, (factor, batch, (h, w), kinds) in CASES.items():
        seed, draws = find_seed(package, factor, batch, kinds)
        end = np.array([random.random(), np.random.rand()])
        gt = np.stack([make_image(rng, (3, h, w)) for _ in range(batch)])
        seed_all(seed)
        kernels = np.zeros((batch, 2, KMAX, KMAX))
        half = np.zeros((batch, 3, h // 2, w // 2), dtype=np.float32)
        before, lr = [], []
        for n in range(batch):
            captured["kernels"], captured["resize"] = [], []
            x = gt[n].astype(np.float32) / np.float32(255)
            y = imgproc.degradation_process(np.ascontiguousarray(x.transpose(1, 2, 0)), factor)
            rec = draws[n]
            assert len(captured["kernels"]) == 2 and len(captured["resize"]) == (2 if rec["half"] == "imresize" else 1)
            for j, k in enumerate(captured["kernels"]):
                blurs = [p for kind, p in rec["ops"] if kind == "blur"]
                assert k.shape == (blurs[j]["ksize"],) * 2, "the package's draws do not describe what the reference ran"
                o = (KMAX - k.shape[0]) // 2
                kernels[n, j, o:o + k.shape[0], o:o + k.shape[0]] = k
            if rec["half"] == "imresize":
                half[n] = np.clip(captured["resize"][0][1], 0, 1)
            pre = captured["resize"][-1][0]
            u8 = np.rint(pre * 255).astype(np.uint8)
            assert ((u8.astype(np.float32) / np.float32(255.)).view(np.uint32) == pre.view(np.uint32)).all()
            before.append(u8)
            lr.append(np.array(y, dtype=np.float32).transpose(2, 0, 1))
            # the oracle, continued from the reference's own half-size image, must land on the same bytes
            mine = BO.before_resize(x, rec, kernels[n], start=half[n] if rec["half"] == "imresize" else None)
            print(f"{name}[{n}]: half {rec['half']} {rec['interp']}, ops {[(k, p if k == 'jpeg' else p['ksize']) for k, p in rec['ops']]}, final q "
                  f"{rec['final_quality']}; oracle vs reference before the resize: {int((mine != u8).sum())} differing bytes")
            assert (mine == u8).all()
        assert np.array_equal(end, np.array([random.random(), np.random.rand()])), "the package's draws leave the streams elsewhere"
        lr = np.stack(lr)
        out.update({f"{name}_gt": gt, f"{name}_seed": np.int64(seed), f"{name}_factor": np.int64(factor), f"{name}_draws": np.array(json.dumps(draws)),
                    f"{name}_end": end, f"{name}_kernels": kernels, f"{name}_half": half, f"{name}_lr": lr})
        for n in range(batch):
            out[f"{name}_before{n}"] = before[n]
    for (h, w) in JPEG_SIZES:
        imgs = np.stack([make_image(rng, (3, h, w)) if i else rng.randint(0, 256, size=(3, h, w)).astype(np.uint8) for i in range(3)])
        trips = np.zeros((3, len(JPEG_QUALITIES), 3, h, w), dtype=np.uint8)
        for i in range(3):
            for j, q in enumerate(JPEG_QUALITIES):
                buf = io.BytesIO()
                Image.fromarray(np.ascontiguousarray(imgs[i].transpose(1, 2, 0))).save(buf, format="JPEG", quality=q)
                trips[i, j] = np.array(Image.open(io.BytesIO(buf.getvalue())).convert("RGB")).transpose(2, 0, 1)
                assert (JO.roundtrip_u8(imgs[i].transpose(1, 2, 0), q).transpose(2, 0, 1) == trips[i, j]).all()
        out[f"jpeg_{h}x{w}_in"], out[f"jpeg_{h}x{w}_out"] = imgs, trips
    path = os.path.join(HERE, "bsrgan_degradation.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= SIZE_LIMIT


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ["SRGAN_REFERENCE"])
