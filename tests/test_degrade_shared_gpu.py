"""What the degradation kernels share (sr_gan_fd_amd/csrc/filter2d.hip, jpeg.hip, degrade.hip), at the smallest shapes where a shared
piece can go wrong: the 8-bit quantiser of three entry points, the tile staging and sliding window under both accumulator types, the
MCU frame of both JPEG round trips."""
import numpy as np
import pytest
import torch

from tests import jpeg_oracle as JO
from tests.test_degradation_gpu import _jpeg_check

pytestmark = pytest.mark.gpu


def test_one_quantiser_behind_three_entry_points():
    """quantize_u8, the Gaussian-noise stage with clip + rounds and the Poisson stage's img_q are the same function of a value: the ties
    (j + 0.5) / 255, which round to even, both clamps and both ends"""
    from sr_gan_fd_amd import imgproc
    vals = np.concatenate([(np.arange(256, dtype=np.float64) + 0.5) / 255, [-0.1, 1.1, 0.0, 1.0]]).astype(np.float32)
    assert vals.size == 260
    want = np.clip(np.rint(vals * np.float32(255)), 0, 255).astype(np.float32) / np.float32(255)
    assert want.dtype == np.float32
    x = torch.from_numpy(vals.reshape(1, 1, 13, 20)).cuda()
    zero = torch.zeros(1, device="cuda")
    got = {"quantize_u8": imgproc.quantize_u8(x),
           "gaussian noise, sigma 0, clip + rounds": imgproc.gaussian_noise_apply(x, torch.randn_like(x), None, zero, zero, True, True),
           "poisson prepare img_q": imgproc.poisson_noise_prepare(x, False)[0]}
    for what, g in got.items():
        g = g.cpu().numpy().reshape(-1)
        assert g.tobytes() == want.tobytes(), (what, int((g != want).sum()))


def _mirror_correlate_f64(x, k):
    """float64 cross-correlation of a float32 plane with mirror padding (no repeat of the edge sample)"""
    r, (h, w) = k.shape[0] // 2, x.shape
    p = np.pad(x.astype(np.float64), r, mode="reflect")
    out = np.zeros((h, w))
    for dy in range(k.shape[0]):
        for dx in range(k.shape[1]):
            out += k[dy, dx] * p[dy:dy + h, dx:dx + w]
    return out


def _kernels(rng, n, k):
    """per-image non-negative k x k kernels, normalised in float32, so that their float64 copies are the same numbers"""
    kk = rng.rand(n, k, k).astype(np.float32)
    return kk / kk.sum(axis=(1, 2), keepdims=True, dtype=np.float32)


@pytest.mark.parametrize("shape,k", [((2, 1, 33, 65), 7), ((1, 1, 13, 13), 25), ((1, 1, 26, 27), 51)])
def test_tile_staging_and_window_under_both_accumulators(shape, k):
    """2 x 2 ragged tiles at k = 7; the mirror limits, where the halo is the whole image: k = 25 at 13 x 13 (the fp64 kernel's largest)
    and k = 51 at 26 x 27 (the fp32 kernel's).  fp64: the float64 correlation rounded once, exactly.  fp32: within k * k * 2^-24 of it,
    the bound on a k * k-term fp32 sum of products whose absolute values sum to at most 1 (image in [0, 1], weights >= 0 of sum 1)."""
    from sr_gan_fd_amd import imgproc
    rng = np.random.RandomState(k)
    x = rng.rand(*shape).astype(np.float32)
    kern = _kernels(rng, shape[0], k)
    want = np.stack([np.stack([_mirror_correlate_f64(x[n, c], kern[n].astype(np.float64)) for c in range(shape[1])]) for n in range(shape[0])])
    got32 = imgproc.filter2d_torch(torch.from_numpy(x).cuda(), torch.from_numpy(kern).cuda()).cpu().numpy()
    bound = k * k * 2.0 ** -24
    if k <= 25:
        k25 = np.zeros((shape[0], 25, 25))
        o = (25 - k) // 2
        k25[:, o:o + k, o:o + k] = kern
        got64 = imgproc.filter2d_mirror_f64(torch.from_numpy(x).cuda(), k25, [k] * shape[0]).cpu().numpy()
        assert got64.dtype == np.float32
        exact = want.astype(np.float32)
        print(f"fp64 {shape} k = {k}: {int((got64 != exact).sum())} values differ from the rounded float64 correlation")
        assert got64.tobytes() == exact.tobytes()
        err = np.abs(got32.astype(np.float64) - got64.astype(np.float64)).max()
    else:
        err = np.abs(got32.astype(np.float64) - want).max()
    print(f"fp32 {shape} k = {k}: max difference {err:.3e}, bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("shape", [(3, 3, 16, 16), (1, 3, 17, 33)])
def test_mcu_frame_of_both_round_trips(shape):
    """three MCUs and one dead wave in the only workgroup; 2 x 3 MCUs with a ragged last row and column"""
    from oracle import degradation_oracle as D
    from sr_gan_fd_amd import imgproc
    torch.manual_seed(shape[-1])
    b = shape[0]
    img = torch.nn.functional.interpolate(torch.rand(b, 3, 6, 7), size=shape[2:], mode="bilinear") * 0.8 + 0.2 * torch.rand(shape)
    quality = torch.empty(b).uniform_(20, 98)
    want = D.diff_jpeg(img, D.quality_to_factor(quality))
    _jpeg_check(imgproc.DiffJPEG().cuda()(img.cuda(), quality.cuda()), want.numpy(), f"DiffJPEG {shape}")
    q = (40, 0, 90) if b == 3 else (75,)
    got = imgproc.jpeg_compression(img.cuda(), q).cpu()
    for n in range(b):
        if q[n] == 0:
            assert got[n].numpy().tobytes() == img[n].numpy().tobytes()              # returned bit for bit
        else:
            assert torch.equal(got[n], torch.from_numpy(JO.roundtrip(img[n].numpy(), q[n]))), (shape, n, q[n])
