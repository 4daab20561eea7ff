"""Writes tests/golden/realesrgan_kernels.npz: the per-image filter kernels the reference project's Real-ESRGAN dataset makes on the host
(Real_ESRGAN/dataset.py:64-133 with imgproc.random_mixed_kernels, imgproc.py:495-576, and generate_sinc_kernel, :579-606), for the
parameters sr_gan_fd_amd.imgproc.blur_kernel_bank is tested at.  Data only.

    python tests/golden/make_golden_realesrgan_kernels.py /path/to/reference        (or SRGAN_REFERENCE in the environment)

Needs scipy (``special.j1``).  The reference's files import cv2 and torchvision, which are not dependencies here; they get empty stand-ins
(the kernel synthesis touches neither), and the dataset's image read is answered with a 4 x 4 black image.

Recorded:
  sweep_*   every kernel family at every size 7, 9, .. 21 and at the corners of the configured parameter ranges (sigma 0.2 / 3 with
            sigma_x != sigma_y for the anisotropic ones, theta -pi / 0.7 / pi, beta 0.5 / 1 / 4 generalized and 1 / 2 plateau, omega pi / 5,
            pi / 3, pi): ``sweep_kind``, ``sweep_ksize``, ``sweep_params`` (sigma_x, sigma_y, theta, beta, omega: blur_kernel_bank's
            arguments), ``sweep_family`` and ``sweep_values``, the reference's float64 outputs at their own k x k size, flattened and
            concatenated in order.  The Gaussian families go through the reference's own ``_random_bivariate_*`` functions (they divide by
            the sum a second time) with ``np.random.uniform`` answering from a script for the duration of the call.
  config    the degradation-model parameters of realesrgan_config.py:46-65, read from that file as a literal (JSON).
  seed<s>_* for two seeds, B = 4: the three float32 tensors the reference's ``DegeneratedImageDataset.__getitem__`` returns, image by
            image after ``random.seed(s)`` / ``np.random.seed(s)``, stacked; the draws as the package's ``realesrgan_kernel_draws`` makes
            them after the same seeding (JSON); and the next draw of either stream after the batch.  Each seed's draws cover a sinc first
            kernel, a delta and a sinc third kernel, a generalized and a plateau kernel.
While it writes, the script checks the package's draws against the reference's kernels through a numpy restatement of the closed form in
include/srganfd.h, and prints how many float32 elements differ."""
import ast
import importlib
import json
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

SIZE_LIMIT = 512 * 1024
SIZES = [7, 9, 11, 13, 15, 17, 19, 21]
SIGMAS = [0.2, 3.0]
THETAS = [-np.pi, 0.7, np.pi]
BETAS = {2: [0.5, 1.0, 4.0], 3: [1.0, 2.0]}
OMEGAS = [np.pi / 5, np.pi / 3, np.pi]
BATCH = 4


def import_reference(ref):
    for name in ("cv2", "torchvision", "torchvision.transforms", "torchvision.transforms.functional", "torchvision.transforms.functional_tensor"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["torchvision.transforms"].functional = sys.modules["torchvision.transforms.functional"]
    sys.modules["torchvision.transforms.functional_tensor"].rgb_to_grayscale = None
    cv2 = sys.modules["cv2"]
    cv2.COLOR_BGR2RGB = 4
    cv2.imread = lambda path: np.zeros((4, 4, 3), dtype=np.uint8)
    cv2.cvtColor = lambda image, code: image
    path = os.path.join(ref, "Real_ESRGAN")
    sys.path.insert(0, path)
    try:
        for name in ("imgproc", "dataset"):
            sys.modules.pop(name, None)
        ip = importlib.import_module("imgproc")
        ds = importlib.import_module("dataset")
    finally:
        sys.path.remove(path)
        for name in ("imgproc", "dataset"):
            sys.modules.pop(name, None)
    ip.image_to_tensor = lambda image, range_norm, half: torch.zeros(3, 4, 4)
    with open(os.path.join(path, "realesrgan_config.py")) as f:
        tree = ast.parse(f.read())
    config = None
    for node in tree.body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == "degradation_model_parameters_dict":
            config = ast.literal_eval(node.value)
    return ip, ds, config


class scripted_uniform:
    """np.random.uniform answers from ``values`` in order (whatever range it is asked for) while the block runs"""

    def __init__(self, values):
        self.values = list(values)

    def __enter__(self):
        self.saved = np.random.uniform
        np.random.uniform = lambda *a, **k: self.values.pop(0)

    def __exit__(self, *exc):
        np.random.uniform = self.saved
        assert exc[0] is not None or not self.values, "the reference drew fewer values than scripted"


def reference_kernel(ip, kind, aniso, k, sx, sy, theta, beta, omega):
    if kind == 4:
        return ip.generate_sinc_kernel(omega, k, padding=False)
    script = [sx] + ([sy, theta] if aniso else [])
    sigma, rot = (0.1, 10.0), (-4.0, 4.0)
    if kind == 1:
        with scripted_uniform(script):
            return ip._random_bivariate_gaussian_kernel(k, sigma, sigma, rot, None, not aniso)
    script += [0.0, beta]                                   # "uniform() < 0.5", then the beta itself
    fn = ip._random_bivariate_generalized_gaussian_kernel if kind == 2 else ip._random_bivariate_plateau_gaussian_kernel
    with scripted_uniform(script):
        return fn(k, sigma, sigma, rot, (0.1, 10.0), None, not aniso)


def restate(rec, kmax):
    """the closed form of include/srganfd.h in numpy float64, centred in kmax x kmax"""
    out = np.zeros((kmax, kmax))
    if rec["kind"] == 0:
        out[kmax // 2, kmax // 2] = 1.0
        return out
    k = rec["ksize"]
    ax = np.arange(k, dtype=np.float64) - k // 2
    x, y = ax[None, :], ax[:, None]
    if rec["kind"] == 4:
        from scipy import special
        w = rec["omega"]
        r = np.sqrt(x * x + y * y)
        with np.errstate(divide="ignore", invalid="ignore"):
            v = w * special.j1(w * r) / (2 * np.pi * r)
        v[k // 2, k // 2] = w * w / (4 * np.pi)
    else:
        c, s, vx, vy = np.cos(rec["theta"]), np.sin(rec["theta"]), rec["sigma_x"] ** 2, rec["sigma_y"] ** 2
        a, b, d = c * c * vx + s * s * vy, c * s * (vx - vy), s * s * vx + c * c * vy
        q = (d * x * x - 2.0 * b * x * y + a * y * y) / (a * d - b * b)
        v = np.exp(-0.5 * q) if rec["kind"] == 1 else np.exp(-0.5 * np.power(q, rec["beta"])) if rec["kind"] == 2 else 1.0 / (np.power(q, rec["beta"]) + 1.0)
    o = (kmax - k) // 2
    out[o:o + k, o:o + k] = v / np.sum(v)
    return out


def sweep_cases():
    """(family, kind, anisotropic, ksize, sigma_x, sigma_y, theta, beta, omega): every family at every size, every corner in some kernel"""
    cases = []
    for i, k in enumerate(SIZES):
        for j, s in enumerate(SIGMAS):
            cases.append(("isotropic", 1, False, k, s, s, 0.0, 0.0, 0.0))
            cases.append(("anisotropic", 1, True, k, s, SIGMAS[1 - j], THETAS[(i + j) % 3], 0.0, 0.0))
        for kind, name in ((2, "generalized"), (3, "plateau")):
            for j, beta in enumerate(BETAS[kind]):
                s = SIGMAS[(i + j) % 2]
                cases.append((name + "_isotropic", kind, False, k, s, s, 0.0, beta, 0.0))
                cases.append((name + "_anisotropic", kind, True, k, s, SIGMAS[1 - (i + j) % 2], THETAS[(i + j + kind) % 3], beta, 0.0))
        for w in OMEGAS:
            cases.append(("sinc", 4, False, k, 0.0, 0.0, 0.0, 0.0, w))
    return cases


def seed_all(s):
    random.seed(s)
    np.random.seed(s)


def covers(draws):
    recs = [r[n] for r in draws for n in ("kernel1", "kernel2")]
    return (any(r["kernel1"]["kind"] == 4 for r in draws) and any(r["sinc_kernel"]["kind"] == 0 for r in draws) and any(r["sinc_kernel"]["kind"] == 4 for r in draws)
            and any(r["kind"] == 2 for r in recs) and any(r["kind"] == 3 for r in recs))


def differing(a64, b64):
    return int((np.asarray(a64, dtype=np.float32).view(np.uint32) != np.asarray(b64, dtype=np.float32).view(np.uint32)).sum())


def main(ref):
    from sr_gan_fd_amd import imgproc as package
    ip, ds, config = import_reference(ref)
    assert config is not None and config["gaussian_kernel_range"] == SIZES
    out = {"config": np.array(json.dumps(config))}
    # ---- the sweep
    cases = sweep_cases()
    values, diff, total = [], 0, 0
    for family, kind, aniso, k, sx, sy, theta, beta, omega in cases:
        v = np.asarray(reference_kernel(ip, kind, aniso, k, sx, sy, theta, beta, omega), dtype=np.float64)
        assert v.shape == (k, k) and np.isfinite(v).all()
        mine = restate(dict(kind=kind, ksize=k, sigma_x=sx, sigma_y=sy, theta=theta, beta=beta, omega=omega), k)
        diff, total = diff + differing(v, mine), total + k * k
        values.append(v.reshape(-1))
    print(f"sweep: {len(cases)} kernels; the closed form in numpy differs from the reference in {diff} of {total} float32 elements")
    out.update(sweep_family=np.array([c[0] for c in cases]), sweep_kind=np.array([c[1] for c in cases], dtype=np.int32),
               sweep_ksize=np.array([c[3] for c in cases], dtype=np.int32), sweep_params=np.array([c[4:] for c in cases], dtype=np.float64),
               sweep_values=np.concatenate(values))
    # ---- seeded batches through the reference's dataset
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "0.png"), "w").close()
        dataset = ds.DegeneratedImageDataset(d, config)
        seeds = []
        for s in range(100000):
            seed_all(s)
            draws = package.realesrgan_kernel_draws(BATCH, config)
            if not covers(draws):
                continue
            end = np.array([random.random(), np.random.rand()])
            seed_all(s)
            items = [dataset[0] for _ in range(BATCH)]
            assert np.array_equal(end, np.array([random.random(), np.random.rand()])), "the package's draws leave the streams elsewhere"
            diff = 0
            for name, key in (("kernel1", "gaussian_kernel1"), ("kernel2", "gaussian_kernel2"), ("sinc_kernel", "sinc_kernel")):
                got = np.stack([it[key].numpy() for it in items])
                assert got.dtype == np.float32 and got.shape == (BATCH, 21, 21)
                mine = np.stack([restate(r[name], 21) for r in draws])
                assert np.abs(got - mine.astype(np.float32)).max() <= 1e-7, "the package's draws do not describe what the reference made"
                diff += differing(got, mine)
                out[f"seed{s}_{key}"] = got
            out[f"seed{s}_draws"], out[f"seed{s}_end"] = np.array(json.dumps(draws)), end
            print(f"seed {s}: kinds {[[r[n]['kind'] for n in ('kernel1', 'kernel2', 'sinc_kernel')] for r in draws]}; closed form vs reference: "
                  f"{diff} differing float32 elements")
            seeds.append(s)
            if len(seeds) == 2:
                break
    out["seeds"] = np.array(seeds, dtype=np.int64)
    path = os.path.join(HERE, "realesrgan_kernels.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= SIZE_LIMIT


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ["SRGAN_REFERENCE"])
