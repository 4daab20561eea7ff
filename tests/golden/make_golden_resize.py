"""Writes tests/golden/image_resize.npz: inputs and, for each case, what the reference project's imgproc.image_resize
(ESRGAN/imgproc.py:202-288) computes on the CPU -- its float32 output and, for each side, the weights, indices and the two
sym_len's of its _calculate_weights_indices (:53-127), captured by wrapping that function at run time.  Data only.

    python tests/golden/make_golden_resize.py /path/to/reference        (or SRGAN_REFERENCE in the environment)

Inputs lie on the u8 grid (x = u8.astype(float32) / float32(255), the expression the tests repeat) and are stored as differences along the
width.  The outputs of the enlarging cases alone would be 0.5 MB of float32 that deflate cannot shrink, so each output is stored as
its distance in float32 units in the last place from tests/resize_oracle.anchor() -- the recorded tables applied in fp64, elementwise
operations only, the same bits on every machine -- which is a few units at most and compresses to almost nothing;
tests/resize_oracle.load_cases adds it back, and this script checks that doing so restores the reference's output bit for bit."""
import importlib
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resize_oracle as RO  # noqa: E402

# name: (shape, scale, antialiasing); every one is a case the reference runs as written
CASES = {
    "q128": ((3, 128, 128), 1 / 4, True), "q97x131": ((3, 97, 131), 1 / 4, True), "h96x120": ((3, 96, 120), 1 / 2, True),
    "t90x75": ((3, 90, 75), 1 / 3, True), "e128x96": ((3, 128, 96), 1 / 8, True), "x2_33x47": ((3, 33, 47), 2, True),
    "x4_40x28": ((3, 40, 28), 4, True), "s03_61x83": ((3, 61, 83), 0.3, True), "s07_50x70": ((3, 50, 70), 0.7, True),
    "s07_50x70_plain": ((3, 50, 70), 0.7, False), "q65x66_plain": ((3, 65, 66), 1 / 4, False), "x3_31x18_plain": ((3, 31, 18), 3, False),
    "q7x9": ((3, 7, 9), 1 / 4, True), "s09_301x203": ((1, 301, 203), 0.9, True), "x15_77x64_2d": ((77, 64), 1.5, True),
}
SIZE_LIMIT = 512 * 1024


def import_reference(ref):
    if "cv2" not in sys.modules:
        sys.modules["cv2"] = types.ModuleType("cv2")
    path = os.path.join(ref, "ESRGAN")
    sys.path.insert(0, path)
    try:
        sys.modules.pop("imgproc", None)
        return importlib.import_module("imgproc")
    finally:
        sys.path.remove(path)


def make_image(rng, shape):
    """smooth structure plus noise, clamped to [0,1], on the u8 grid"""
    h, w = shape[-2:]
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    planes = []
    for _ in range(int(np.prod(shape[:-2], dtype=np.int64))):
        f, p = rng.uniform(0.5, 4.0, size=3), rng.uniform(0, 2 * np.pi, size=3)
        img = 0.5 + 0.25 * np.sin(2 * np.pi * f[0] * xx + p[0]) * np.cos(2 * np.pi * f[1] * yy + p[1]) + 0.2 * np.sin(2 * np.pi * f[2] * (xx + yy) + p[2])
        planes.append(img + rng.normal(0, 0.03, size=(h, w)))
    return np.rint(np.clip(np.stack(planes).reshape(shape), 0, 1) * 255).astype(np.uint8)


def delta_x(a):
    d = a.copy()
    d[..., 1:] = a[..., 1:] - a[..., :-1]
    assert (np.cumsum(d, axis=-1, dtype=a.dtype) == a).all()
    return d


def main(ref):
    imgproc = import_reference(ref)
    captured = []
    tables = imgproc._calculate_weights_indices

    def tables_w(*a, **k):
        r = tables(*a, **k)
        captured.append(r)
        return r

    imgproc._calculate_weights_indices = tables_w
    rng = np.random.RandomState(20240911)
    out = {"names": np.array(list(CASES))}
    for name, (shape, scale, aa) in CASES.items():
        u8 = make_image(rng, shape)
        x = u8.astype(np.float32) / np.float32(255)          # the expression the tests repeat
        del captured[:]
        y = imgproc.image_resize(torch.from_numpy(x), scale, aa).numpy()
        (wh, ih, hs, he), (ww, iw, ws, we) = captured
        assert y.dtype == np.float32 and y.shape == shape[:-2] + (math.ceil(shape[-2] * scale), math.ceil(shape[-1] * scale))
        wh, ww, ih, iw = wh.numpy(), ww.numpy(), ih.numpy(), iw.numpy()
        assert wh.dtype == ww.dtype == np.float32 and (ih == np.rint(ih)).all() and (iw == np.rint(iw)).all()
        ih, iw = ih.astype(np.int32), iw.astype(np.int32)
        base = RO.anchor(x, wh, ih[:, 0].astype(np.int64) - hs, ww, iw[:, 0].astype(np.int64) - ws)
        ulps = RO.ordered(y) - RO.ordered(base)
        assert np.abs(ulps).max() < 2 ** 31
        assert (RO.from_ordered(RO.ordered(base) + ulps).reshape(y.shape).view(np.uint32) == y.view(np.uint32)).all()
        b = RO.bound_for(shape[-2], shape[-1], scale, aa)
        err = np.abs(y.astype(np.float64) - RO.resize(x, scale, aa)).max()
        print(f"{name}: {shape} x {scale:.4g} -> {y.shape}, taps {wh.shape[1]} / {ww.shape[1]}, sym_len {hs} {he} {ws} {we}, "
              f"|ulps| max {np.abs(ulps).max()}, reference vs oracle {err:.2e} = {err / b:.3f} B")
        out.update({f"{name}_input_dx": delta_x(u8), f"{name}_scale": np.float64(scale), f"{name}_antialiasing": np.bool_(aa),
                    f"{name}_output_ulps": ulps.astype(np.int32), f"{name}_sym": np.array([hs, he, ws, we], dtype=np.int32),
                    f"{name}_weights_h": wh, f"{name}_indices_h": ih, f"{name}_weights_w": ww, f"{name}_indices_w": iw})
    path = os.path.join(HERE, "image_resize.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= SIZE_LIMIT
    got = RO.load_cases(path)
    assert list(got) == list(CASES)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ["SRGAN_REFERENCE"])
