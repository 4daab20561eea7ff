"""BSRGAN's blind degradation on the GPU (sr_gan_fd_amd/csrc/jpeg.hip, filter2d.hip, imgproc.degradation_process_bsrgan and the prefetcher's
``synthesize_lr_bsrgan``) against the reference's recorded results (tests/golden/bsrgan_degradation.npz) and the numpy oracles of
tests/jpeg_oracle.py and tests/bsrgan_degradation_oracle.py.  Needs numpy and the fixture only.

JPEG: integer arithmetic, so ``torch.equal`` -- no tolerance.
Blur: the kernel sums in fp64 with fused multiply-adds, column of the filter by column; the oracle sums unfused, in either order.  All
three round once to float32 and are expected to give the same bits; where an fp64 sum lies within 1e-16 relative of the midpoint of two
floats they may not.  The test allows BLUR_MISMATCH_CAP = 2 values per case to differ, by one unit in the last place and no more, and checks
that the oracle's own two summation orders differ in no more than that many places on the same inputs (so the inputs are not the cause).
Pipeline: everything before the final ``image_resize`` is expected to be exact, so the LR image is held to the bound of that resize alone,
with the logic of tests/test_image_resize_gpu.py: B = resize_oracle.bound_for(...) from the tables, kernel vs the fp64 oracle <= B, kernel vs
the reference's recorded float32 LR <= 2 B, both widened by 2 P S delta for a measured table difference delta <= 2^-20 (expected 0)."""
import math
import os
import random

import numpy as np
import pytest
import torch

from tests import bsrgan_degradation_oracle as BO
from tests import jpeg_oracle as JO
from tests import resize_oracle as RO

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DELTA_MAX = 2.0 ** -20
BLUR_MISMATCH_CAP = 2


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return BO.load_fixture(os.path.join(golden_dir, "bsrgan_degradation.npz"))


def seed_all(s):
    random.seed(s)
    np.random.seed(s)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def as_float(u8):
    return np.asarray(u8).astype(np.float32) / np.float32(255.)


def jpeg(x, quality):
    from sr_gan_fd_amd.imgproc import jpeg_compression
    y = jpeg_compression(x, quality)
    torch.cuda.synchronize()
    return y


# ---- JPEG ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(16, 16), (9, 23), (17, 33), (37, 52)])
def test_jpeg_against_fixture_and_oracle(fixture, size):
    inputs, outputs = fixture["jpeg"][size]
    col = {q: j for j, q in enumerate(fixture["qualities"])}
    x = as_float(inputs)
    got = jpeg(gpu(x), (30, 50, 95))
    assert got.dtype == torch.float32 and got.shape == (3, 3) + size
    for i, q in enumerate((30, 50, 95)):
        assert torch.equal(got[i].cpu(), torch.from_numpy(as_float(outputs[i, col[q]]))), (size, q)
        assert torch.equal(got[i].cpu(), torch.from_numpy(JO.roundtrip(x[i], q))), (size, q)
    x[1] += np.float32(1e-3)                                      # off the 8-bit grid: a requantised copy would show
    dev = gpu(x)
    for quality in ((47, 0, 75), torch.tensor([47, 0, 75], dtype=torch.int32), torch.tensor([47, 0, 75], dtype=torch.int32, device=DEV)):
        got = jpeg(dev, quality)
        assert torch.equal(got[0].cpu(), torch.from_numpy(as_float(outputs[0, col[47]])))
        assert torch.equal(got[1], dev[1]) and got[1].cpu().numpy().tobytes() == x[1].tobytes()
        assert torch.equal(got[2].cpu(), torch.from_numpy(JO.roundtrip(x[2], 75)))
    assert torch.equal(jpeg(dev[0], 47), got[0])                  # (3, H, W) in, (3, H, W) out


def test_jpeg_random_inputs_against_oracle():
    rng = np.random.RandomState(5)
    for shape, quality in (((1, 3, 8, 8), (61,)), ((2, 3, 40, 56), (37, 88)), ((2, 3, 1, 1), (50, 95)), ((1, 3, 6, 4), (30,)), ((1, 3, 50, 3), (75,))):
        x = rng.uniform(-0.2, 1.2, size=shape).astype(np.float32)           # any range: clipped, then rounded half to even
        got = jpeg(gpu(x), quality).cpu()
        for i, q in enumerate(quality):
            want = JO.roundtrip(x[i], q)
            assert torch.equal(got[i], torch.from_numpy(want)), (shape, q, int((got[i].numpy() != want).sum()))


def test_jpeg_refuses_bad_arguments():
    from sr_gan_fd_amd import _abi as A
    x = torch.zeros(2, 3, 16, 16, device=DEV)
    for bad in ((50, 101), (-1, 50), (50,), 101):
        with pytest.raises(A.SrganfdError):
            jpeg(x, bad)
    with pytest.raises(A.SrganfdError):
        jpeg(torch.zeros(2, 1, 16, 16, device=DEV), 50)


# ---- blur ------------------------------------------------------------------------------------------------------------------------------
def random_kernels(rng, sizes, kmax=25):
    """positive kernels of sum 1, NOT symmetric (a flipped or transposed filter would show), each centred in kmax x kmax"""
    k = np.zeros((len(sizes), kmax, kmax))
    for n, s in enumerate(sizes):
        if s:
            v = rng.uniform(0.1, 1.0, size=(s, s)) * np.exp(-np.linspace(-2, 2, s) ** 2)[None, :]
            o = (kmax - s) // 2
            k[n, o:o + s, o:o + s] = v / v.sum()
    return k


def ulps_apart(a, b):
    return np.abs(RO.ordered(a) - RO.ordered(b))


def check_blur(x, kernels, sizes):
    from sr_gan_fd_amd.imgproc import filter2d_mirror_f64
    got = filter2d_mirror_f64(gpu(x), kernels, sizes)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == x.shape
    for n, s in enumerate(sizes):
        if s == 0:
            assert got[n].tobytes() == x[n].tobytes()
            continue
        k = BO.trim_kernel(kernels[n], s)
        want, other = BO.blur(x[n], k), BO.blur(x[n], k, columns_first=True)
        d_orders, d = ulps_apart(want, other), ulps_apart(got[n], want)
        print(f"blur k = {s} on {x[n].shape}: kernel vs oracle {int((d != 0).sum())} values differ (largest {int(d.max())} ulp); "
              f"the oracle's two summation orders {int((d_orders != 0).sum())}")
        assert (d_orders != 0).sum() <= BLUR_MISMATCH_CAP
        assert d.max() <= 1 and (d != 0).sum() <= BLUR_MISMATCH_CAP


def test_blur_three_sizes_in_one_launch():
    rng = np.random.RandomState(21)
    x = rng.rand(3, 3, 32, 40).astype(np.float32)
    check_blur(x, random_kernels(rng, (7, 25, 0)), (7, 25, 0))


def test_blur_at_the_mirror_limit_and_across_tiles():
    rng = np.random.RandomState(22)
    check_blur(rng.rand(1, 3, 13, 13).astype(np.float32), random_kernels(rng, (25,)), (25,))
    check_blur(rng.rand(2, 1, 37, 70).astype(np.float32), random_kernels(rng, (9, 3), kmax=9), (9, 3))      # two tiles each way, kmax < 25


def test_blur_refuses_what_does_not_fit():
    from sr_gan_fd_amd import _abi as A
    from sr_gan_fd_amd.imgproc import filter2d_mirror_f64
    rng = np.random.RandomState(23)
    with pytest.raises(A.SrganfdError):
        filter2d_mirror_f64(torch.zeros(1, 3, 12, 12, device=DEV), random_kernels(rng, (25,)), (25,))
    with pytest.raises(A.SrganfdError):
        filter2d_mirror_f64(torch.zeros(1, 3, 32, 32, device=DEV), random_kernels(rng, (7,)), (8,))


def test_half_size_step_matches_its_restatement():
    """``interpolate(scale_factor=0.5)`` is what stands in for ``cv2.resize`` to half size.  Area and bilinear multiply by powers of two
    only, so the float32 restatement is exact whatever the compiler fuses; the bicubic one (taps -0.09375, 0.59375, 0.59375, -0.09375, sum
    of |taps| S = 1.375, P = 4 per pass) is two float32 evaluations of the same sums: within 2 B, B = 2 (P + 3) 2^-24 S^2 as in resize_oracle"""
    from sr_gan_fd_amd.imgproc import interpolate
    x = np.random.RandomState(31).rand(2, 3, 26, 38).astype(np.float32)
    for interp, mode in ((3, "area"), (1, "bilinear"), (2, "bicubic")):
        got = interpolate(gpu(x), scale_factor=0.5, mode=mode).cpu().numpy()
        want = np.stack([BO.half_cv2(x[i], interp) for i in range(2)])
        err = float(np.abs(got.astype(np.float64) - want).max())
        print(f"half size, {mode}: kernel vs restatement {err:.3e}")
        if interp == 2:
            assert err <= 2 * (2 * (4 + 3) * RO.EPS32 * 1.375 ** 2)
        else:
            assert np.array_equal(got, want)


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------------
def degrade(gt, factor, draws=None):
    from sr_gan_fd_amd.imgproc import degradation_process_bsrgan
    y = degradation_process_bsrgan(gt, factor, draws=draws)
    torch.cuda.synchronize()
    return y


@pytest.fixture(scope="module")
def outputs(fixture):
    """every fixture case through the GPU once, with the recorded draws"""
    return {name: degrade(gpu(c["gt"]), c["factor"], c["draws"]) for name, c in fixture["cases"].items()}


def resize_bounds(h, w, scale):
    """(B, widening) of the final image_resize, as tests/test_image_resize_gpu.py derives them"""
    from sr_gan_fd_amd.imgproc import _resize_tables_host
    orc = [RO.tables(n, math.ceil(n * scale), scale, True) for n in (h, w)]
    mine = [_resize_tables_host(n, math.ceil(n * scale), scale, True) for n in (h, w)]
    delta = max(RO.table_delta(m[0].numpy(), m[1].numpy().astype(np.int64), o[0], o[1]) for m, o in zip(mine, orc))
    assert delta <= DELTA_MAX
    p = max(t[0].shape[1] for t in orc)
    s = max(float(np.abs(t[0].astype(np.float64)).sum(1).max()) for t in orc)
    return RO.bound(orc[0][0], orc[1][0]), 2 * p * s * delta


def check_lr(what, got, c, n):
    """image n of case c: against the fp64 oracle run on the package's own kernels (<= B) and against the reference's recorded LR (<= 2 B)"""
    from sr_gan_fd_amd.imgproc import bsrgan_blur_kernels
    rec = c["draws"][n]
    kernels, _ = bsrgan_blur_kernels([rec], c["factor"])
    want, _ = BO.degrade(c["gt"][n], rec, kernels[0])
    h, w = c["before"][n].shape[-2:]
    b, widen = resize_bounds(h, w, 1 / rec["sf"])
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == want.shape == c["lr"][n].shape
    err_o, err_r = float(np.abs(got - want).max()), float(np.abs(got - c["lr"][n].astype(np.float64)).max())
    print(f"{what}[{n}] (half-step {rec['half']}): vs oracle {err_o:.3e} = {err_o / b:.3f} B, vs the recorded reference {err_r:.3e} = {err_r / b:.3f} B")
    assert err_o <= b + widen
    assert err_r <= 2 * b + widen


@pytest.mark.parametrize("name,n", [("x2_32x48", 0), ("x2_32x48", 1), ("x4_64x64", 0), ("x4_64x64", 1), ("x4_64x64", 2), ("x4_64x64", 3)])
def test_degradation_with_recorded_draws(fixture, outputs, name, n):
    """x4_64x64 is a mixed batch: images 0, 1 stay at full size, 2 takes the cv2.resize half-step, 3 the image_resize one"""
    c = fixture["cases"][name]
    got = outputs[name]
    assert got.dtype == torch.float32 and got.is_cuda and got.shape == (len(c["draws"]), 3, c["gt"].shape[2] // c["factor"], c["gt"].shape[3] // c["factor"])
    check_lr(name, got[n], c, n)


def test_degradation_sub_batches_do_not_depend_on_the_batch(fixture, outputs):
    """only the half-step images, only the others, one image: the same bits as inside the mixed batch"""
    c = fixture["cases"]["x4_64x64"]
    gt = gpu(c["gt"])
    for idx in ([2, 3], [0, 1], [3], [1, 2]):
        got = degrade(gt[idx], 4, [c["draws"][i] for i in idx])
        assert torch.equal(got, outputs["x4_64x64"][idx]), idx


@pytest.mark.parametrize("name", ["x2_32x48", "x4_64x64"])
def test_degradation_draws_its_own_numbers_like_the_reference(fixture, outputs, name):
    c = fixture["cases"][name]
    seed_all(c["seed"])
    got = degrade(gpu(c["gt"]), c["factor"])
    assert random.random() == c["end"][0] and np.random.rand() == c["end"][1]
    assert torch.equal(got, outputs[name])


def test_degradation_is_stable(fixture, outputs):
    for name, c in fixture["cases"].items():
        assert torch.equal(degrade(gpu(c["gt"]), c["factor"], c["draws"]), outputs[name])


def test_degradation_refuses_bad_batches():
    from sr_gan_fd_amd import _abi as A
    with pytest.raises(ValueError):
        degrade(torch.zeros(1, 3, 24, 64, device=DEV), 4)
    with pytest.raises(A.SrganfdError):
        degrade(torch.zeros(1, 1, 64, 64, device=DEV), 4)


def test_prefetcher_synthesizes_lr(fixture):
    from sr_gan_fd_amd.dataset import CUDAPrefetcher
    c = fixture["cases"]["x4_64x64"]
    gt = torch.from_numpy(c["gt"])
    given = torch.rand(4, 3, 16, 16)
    loader = [{"gt": gt}, {"gt": gt, "lr": given}, {"gt": gt}]
    seed_all(123)
    want = [degrade(gt.to(DEV), 4), degrade(gt.to(DEV), 4)]
    seed_all(123)
    p = CUDAPrefetcher(loader, DEV, synthesize_lr_bsrgan=dict(upscale_factor=4, jpeg_prob=0.9, scale2_prob=0.25))
    batches = [p.next(), p.next(), p.next()]
    torch.cuda.synchronize()
    assert p.next() is None
    assert batches[0]["lr"].shape == (4, 3, 16, 16) and batches[0]["lr"].is_cuda
    assert torch.equal(batches[0]["lr"], want[0]) and torch.equal(batches[2]["lr"], want[1])
    assert torch.equal(batches[1]["lr"].cpu(), given)                                 # a batch that brings its LR keeps it (and draws nothing)
    assert all(torch.equal(b["gt"].cpu(), gt) for b in batches)
