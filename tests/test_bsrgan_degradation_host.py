"""The host side of BSRGAN's blind degradation (sr_gan_fd_amd/imgproc.py: bsrgan_degradation_draws, bsrgan_blur_kernels, the argument checks
of degradation_process_bsrgan / jpeg_compression / CUDAPrefetcher) and the two numpy oracles the GPU tests rely on, against
tests/golden/bsrgan_degradation.npz (tests/golden/make_golden_bsrgan_degradation.py: the reference's degradation_process run on seeded
inputs).  No GPU.

What "exact" means for the pipeline oracle: everything up to the final ``image_resize`` is integer or correctly rounded arithmetic, and the
oracle reproduces the uint8 image the reference's last JPEG decoded to with 0 differing bytes.  The final ``image_resize`` is float32 torch
code in the reference and fp64 in tests/resize_oracle.py, so the LR image itself is compared within resize_oracle's derived bound B (one
float32 evaluation around the exact value).  The same holds for the ``image_resize`` half-size step in the middle of one case: the oracle's own
half-size image lies within B of the reference's recorded one, and the chain is checked exactly from the recorded one.

Blur kernels: the package's numpy restatement against the recorded scipy-built kernels, largest difference relative to the recorded
entry over the non-zero entries.  Measured when the fixture was made: 0 for every isotropic kernel, 5.4e-14 at most for the anisotropic ones
(the bivariate normal density written out vs scipy's eigen-decomposition); asserted at twice that."""
import io
import json
import os
import random

import numpy as np
import pytest
import torch

from tests import bsrgan_degradation_oracle as BO
from tests import jpeg_oracle as JO
from tests import resize_oracle as RO

KERNEL_REL_MEASURED = 5.4e-14


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return BO.load_fixture(os.path.join(golden_dir, "bsrgan_degradation.npz"))


def seed_all(s):
    random.seed(s)
    np.random.seed(s)


def test_fixture_covers_the_cases(fixture):
    assert set(fixture["jpeg"]) == {(16, 16), (9, 23), (17, 33), (37, 52)} and fixture["qualities"] == [30, 47, 50, 95]
    x2, x4 = fixture["cases"]["x2_32x48"], fixture["cases"]["x4_64x64"]
    assert x2["factor"] == 2 and x2["gt"].shape[1:] == (3, 32, 48) and x4["factor"] == 4 and x4["gt"].shape[1:] == (3, 64, 64)
    assert {r["half"] for r in x4["draws"]} == {None, "imresize", "cv2"} and {r["half"] for r in x2["draws"]} == {None}


def test_jpeg_oracle_equals_recorded_round_trips(fixture):
    for (h, w), (inputs, outputs) in fixture["jpeg"].items():
        for i in range(inputs.shape[0]):
            for j, q in enumerate(fixture["qualities"]):
                got = JO.roundtrip_u8(inputs[i].transpose(1, 2, 0), q).transpose(2, 0, 1)
                assert np.array_equal(got, outputs[i, j]), (h, w, i, q, int((got != outputs[i, j]).sum()))


def test_jpeg_oracle_equals_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.RandomState(7)
    # the fixture's sizes, even heights that are no multiple of 16 (the bottom chroma row is a real average there), planes too narrow for
    # the triangle filter (ceil(w / 2) <= 2: the library repeats them), single rows and columns
    for (h, w) in [(16, 16), (9, 23), (17, 33), (37, 52), (8, 8), (4, 6), (40, 1), (1, 40), (100, 5), (2, 3), (1, 1), (7, 2)]:
        yy, xx = np.mgrid[0:h, 0:w]
        smooth = np.stack([(128 + 100 * np.sin(xx / 7. + c) * np.cos(yy / 5.)).clip(0, 255) for c in range(3)], -1).astype(np.uint8)
        for img in (rng.randint(0, 256, (h, w, 3)).astype(np.uint8), smooth):
            for q in (30, 47, 50, 95):
                buf = io.BytesIO()
                Image.fromarray(img).save(buf, format="JPEG", quality=q)
                want = np.array(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
                got = JO.roundtrip_u8(img, q)
                assert np.array_equal(got, want), (h, w, q, int((got != want).sum()))


def test_jpeg_oracle_float_interface():
    x = np.random.RandomState(3).uniform(-0.2, 1.2, size=(3, 9, 23)).astype(np.float32)
    assert JO.roundtrip(x, 0).tobytes() == x.tobytes()                              # quality 0: untouched
    y = JO.roundtrip(x, 50)
    assert y.dtype == np.float32 and y.shape == x.shape
    u8 = np.rint(y * 255).astype(np.uint8)
    assert ((u8.astype(np.float32) / np.float32(255.)).view(np.uint32) == y.view(np.uint32)).all()


@pytest.mark.parametrize("name", ["x2_32x48", "x4_64x64"])
def test_draws_reproduce_the_recorded_ones(fixture, name):
    """factor 2 draws no scale2 number (the reference's ``upscale_factor == 4 and ...`` short circuit); both streams end where the
    reference left them (the next draw of each was recorded)"""
    from sr_gan_fd_amd.imgproc import bsrgan_degradation_draws
    c = fixture["cases"][name]
    seed_all(c["seed"])
    draws = bsrgan_degradation_draws(len(c["draws"]), c["factor"], 0.9, 0.25)
    assert json.loads(json.dumps(draws)) == json.loads(json.dumps(c["draws"]))
    assert draws == c["draws"]
    assert random.random() == c["end"][0] and np.random.rand() == c["end"][1]


def test_draws_short_circuit_and_probabilities():
    from sr_gan_fd_amd.imgproc import bsrgan_degradation_draws
    seed_all(5)
    state = np.random.get_state()[1].copy()
    d2 = bsrgan_degradation_draws(8, 2, 0.9, 1.0)
    assert all(r["half"] is None and r["sf"] == 2 for r in d2)
    assert (np.random.get_state()[1] == state).all()                                # factor 2 never touches np.random
    d4 = bsrgan_degradation_draws(8, 4, 0.0, 1.0)
    assert all(r["half"] in ("cv2", "imresize") and r["sf"] == 2 for r in d4)
    assert all(p == 0 for r in d4 for kind, p in r["ops"] if kind == "jpeg")         # jpeg_prob 0: always a miss
    for r in d2 + d4:
        assert sorted(r["order"]) == list(range(6)) and [k for k, _ in r["ops"]].count("blur") == 2 and len(r["ops"]) == 3
        assert [k for k, _ in r["ops"]] == [("jpeg" if i == 5 else "blur") for i in r["order"] if i in (0, 1, 5)]
        assert 30 <= r["final_quality"] <= 95 and all(7 <= p["ksize"] <= 25 and p["ksize"] % 2 for k, p in r["ops"] if k == "blur")


@pytest.mark.parametrize("name", ["x2_32x48", "x4_64x64"])
def test_blur_kernels_against_recorded_scipy_kernels(fixture, name):
    from sr_gan_fd_amd.imgproc import bsrgan_blur_kernels
    c = fixture["cases"][name]
    kernels, ksize = bsrgan_blur_kernels(c["draws"], c["factor"])
    assert kernels.dtype == np.float64 and kernels.shape == c["kernels"].shape and ksize.dtype == np.int32
    worst = 0.0
    for n, rec in enumerate(c["draws"]):
        blurs = [p for kind, p in rec["ops"] if kind == "blur"]
        for j, p in enumerate(blurs):
            want, got = c["kernels"][n, j], kernels[n, j]
            assert ksize[n, j] == p["ksize"]
            assert ((want != 0) == (got != 0)).all()                                 # the same support, centred, zeros around it
            nz = want != 0
            worst = max(worst, float((np.abs(got - want)[nz] / want[nz]).max()))
            assert abs(got.sum() - 1) <= 1e-15
            assert np.abs(got - got[::-1, ::-1]).max() <= 1e-17                      # point-symmetric: convolution = correlation
    print(f"{name}: largest relative kernel difference {worst:.2e}")
    assert worst <= 2 * KERNEL_REL_MEASURED
    with pytest.raises(ValueError):
        bsrgan_blur_kernels(c["draws"], c["factor"] + 1)


@pytest.mark.parametrize("name", ["x2_32x48", "x4_64x64"])
def test_pipeline_oracle_reproduces_the_reference(fixture, name):
    c = fixture["cases"][name]
    for n, rec in enumerate(c["draws"]):
        start = None
        if rec["half"] == "imresize":
            mine = BO.half_step(c["gt"][n], rec)
            b = RO.bound_for(c["gt"].shape[-2], c["gt"].shape[-1], 0.5, True)
            err = float(np.abs(mine.astype(np.float64) - c["half"][n]).max())
            print(f"{name}[{n}]: oracle's half-size image vs the reference's {err:.2e} (B {b:.2e})")
            assert err <= b + 2.0 ** -24                                             # + the rounding of the oracle's own value to float32
            start = c["half"][n]
        before = BO.before_resize(c["gt"][n], rec, c["kernels"][n], start)
        assert np.array_equal(before, c["before"][n]), (n, int((before != c["before"][n]).sum()))
        lr, b = BO.degrade(c["gt"][n], rec, c["kernels"][n], start)
        err = float(np.abs(lr - c["lr"][n].astype(np.float64)).max())
        print(f"{name}[{n}]: oracle's LR vs the reference's {err:.2e} = {err / b:.3f} B")
        assert lr.shape == c["lr"][n].shape and err <= b


def test_pipeline_oracle_with_package_kernels(fixture):
    """the kernels the package builds differ from scipy's by 1e-13 relative at most: the blurred float32 values, and with them every byte, stay"""
    from sr_gan_fd_amd.imgproc import bsrgan_blur_kernels
    c = fixture["cases"]["x2_32x48"]
    kernels, _ = bsrgan_blur_kernels(c["draws"], c["factor"])
    for n, rec in enumerate(c["draws"]):
        assert np.array_equal(BO.before_resize(c["gt"][n], rec, kernels[n]), c["before"][n])


def test_half_cv2_restatements():
    x = np.random.RandomState(11).rand(2, 8, 12).astype(np.float32)
    ones = np.ones((1, 6, 10), dtype=np.float32)
    for interp in (1, 2, 3):
        y = BO.half_cv2(x, interp)
        assert y.dtype == np.float32 and y.shape == (2, 4, 6)
        assert np.array_equal(BO.half_cv2(ones, interp), np.ones((1, 3, 5), dtype=np.float32))       # the taps sum to 1 exactly
    want = x.astype(np.float64).reshape(2, 4, 2, 6, 2).mean((2, 4))
    assert np.abs(BO.half_cv2(x, 3) - want).max() <= 2.0 ** -23 and np.abs(BO.half_cv2(x, 1) - want).max() <= 2.0 ** -23


def test_argument_errors_without_a_gpu():
    from sr_gan_fd_amd import _abi as A
    from sr_gan_fd_amd.imgproc import degradation_process_bsrgan, jpeg_compression
    for shape, factor in (((1, 3, 62, 66), 4), ((1, 3, 63, 64), 4), ((1, 3, 33, 48), 2), ((1, 3, 48, 24), 4), ((1, 3, 12, 40), 2), ((1, 3, 40, 12), 1)):
        with pytest.raises(ValueError):
            degradation_process_bsrgan(torch.zeros(shape), factor)
    with pytest.raises(ValueError):
        degradation_process_bsrgan(torch.zeros(1, 3, 64, 64), 0)
    with pytest.raises(ValueError):
        degradation_process_bsrgan(torch.zeros(2, 3, 64, 64), 4, draws=[])             # draws for another batch
    state = random.getstate()
    with pytest.raises(A.SrganfdError):
        degradation_process_bsrgan(torch.zeros(1, 3, 64, 64), 4)                        # a CPU tensor: no fallback
    assert random.getstate() == state                                                  # and nothing was drawn for it
    with pytest.raises(A.SrganfdError):
        degradation_process_bsrgan(torch.zeros(3, 64, 64), 4)
    with pytest.raises(A.SrganfdError):
        jpeg_compression(torch.zeros(1, 3, 16, 16), 50)


def test_entry_points_validate_their_arguments():
    from sr_gan_fd_amd import _abi as A
    L = A.lib()
    assert A.ABI_VERSION == 7 and L.srganfd_abi_version() == 7
    assert L.srganfd_jpeg_workspace_bytes(2, 16, 16) == 2 * 384 and L.srganfd_jpeg_workspace_bytes(1, 17, 33) == 2 * 3 * 384
    assert L.srganfd_jpeg_workspace_bytes(0, 16, 16) == -1 and L.srganfd_jpeg_workspace_bytes(1, 0, 16) == -1
    A.set_dry_run(True)
    try:
        x, y = torch.zeros(2, 3, 12, 12), torch.zeros(2, 3, 12, 12)
        ws = torch.zeros(2 * 384, dtype=torch.uint8)
        q = np.array([50, 0], dtype=np.int32)
        jpeg = lambda *a: L.srganfd_jpeg_roundtrip(*a, 0)
        assert jpeg(x.data_ptr(), 2, 3, 12, 12, q.ctypes.data, q.ctypes.data, ws.data_ptr(), y.data_ptr()) == 0
        assert jpeg(x.data_ptr(), 2, 3, 1, 1, q.ctypes.data, None, ws.data_ptr(), y.data_ptr()) == 0          # smaller than one MCU
        assert jpeg(None, 2, 3, 12, 12, q.ctypes.data, None, ws.data_ptr(), y.data_ptr()) == -1
        assert jpeg(x.data_ptr(), 2, 3, 12, 12, None, None, ws.data_ptr(), y.data_ptr()) == -1
        assert jpeg(x.data_ptr(), 2, 3, 12, 12, q.ctypes.data, None, None, y.data_ptr()) == -1
        assert jpeg(x.data_ptr(), 2, 3, 12, 12, q.ctypes.data, None, ws.data_ptr(), None) == -1
        assert jpeg(x.data_ptr(), 2, 1, 12, 12, q.ctypes.data, None, ws.data_ptr(), y.data_ptr()) == -1       # c != 3
        assert jpeg(x.data_ptr(), 2, 3, 0, 12, q.ctypes.data, None, ws.data_ptr(), y.data_ptr()) == -1
        assert jpeg(x.data_ptr(), 0, 3, 12, 12, q.ctypes.data, None, ws.data_ptr(), y.data_ptr()) == -1
        assert jpeg(x.data_ptr(), 2, 3, 12, 12, q.ctypes.data, None, ws.data_ptr(), x.data_ptr()) == -1       # in place
        for bad in (101, -1):
            qb = np.array([50, bad], dtype=np.int32)
            assert jpeg(x.data_ptr(), 2, 3, 12, 12, qb.ctypes.data, qb.ctypes.data, ws.data_ptr(), y.data_ptr()) == -1
            assert "quality" in L.srganfd_last_error().decode()
        k = torch.zeros(2, 25, 25, dtype=torch.float64)
        blur = lambda *a: L.srganfd_filter2d_mirror_f64(*a, 0)
        ks = np.array([23, 0], dtype=np.int32)
        assert blur(x.data_ptr(), k.data_ptr(), 25, ks.ctypes.data, ks.ctypes.data, 2, 3, 12, 12, y.data_ptr()) == 0   # 12 > 23 // 2
        ks25 = np.array([25, 0], dtype=np.int32)
        assert blur(x.data_ptr(), k.data_ptr(), 25, ks25.ctypes.data, ks25.ctypes.data, 2, 3, 12, 12, y.data_ptr()) == -1   # 12 x 12 under k = 25
        assert blur(x.data_ptr(), k.data_ptr(), 25, ks25.ctypes.data, ks25.ctypes.data, 2, 3, 13, 13, y.data_ptr()) == 0    # the limit
        assert blur(x.data_ptr(), k.data_ptr(), 25, ks.ctypes.data, None, 2, 3, 12, 12, y.data_ptr()) == -1                 # sizes unseen: kmax decides
        for bad in (8, 27, 1, -3):
            kb = np.array([7, bad], dtype=np.int32)
            assert blur(x.data_ptr(), k.data_ptr(), 25, kb.ctypes.data, kb.ctypes.data, 2, 3, 40, 40, y.data_ptr()) == -1
        for kmax in (26, 27, 1):
            assert blur(x.data_ptr(), k.data_ptr(), kmax, ks.ctypes.data, ks.ctypes.data, 2, 3, 40, 40, y.data_ptr()) == -1
        assert blur(None, k.data_ptr(), 25, ks.ctypes.data, ks.ctypes.data, 2, 3, 40, 40, y.data_ptr()) == -1
        assert blur(x.data_ptr(), None, 25, ks.ctypes.data, ks.ctypes.data, 2, 3, 40, 40, y.data_ptr()) == -1
        assert blur(x.data_ptr(), k.data_ptr(), 25, None, None, 2, 3, 40, 40, y.data_ptr()) == -1
        assert blur(x.data_ptr(), k.data_ptr(), 25, ks.ctypes.data, ks.ctypes.data, 2, 3, 40, 40, x.data_ptr()) == -1
        assert blur(x.data_ptr(), k.data_ptr(), 25, ks.ctypes.data, ks.ctypes.data, 2, 0, 40, 40, y.data_ptr()) == -1
    finally:
        A.set_dry_run(False)


def test_prefetcher_argument_checks(monkeypatch):
    from sr_gan_fd_amd import dataset as D

    class Stream:
        def __init__(self, device=None):
            pass

    monkeypatch.setattr(torch.cuda, "Stream", Stream)
    monkeypatch.setattr(D.CUDAPrefetcher, "reset", lambda self: None)                  # no batch is staged: only the constructor runs
    with pytest.raises(ValueError):
        D.CUDAPrefetcher([], "cpu", synthesize_lr=4, synthesize_lr_bsrgan=dict(upscale_factor=4))
    with pytest.raises(ValueError):
        D.CUDAPrefetcher([], "cpu", synthesize_lr_bsrgan=dict(jpeg_prob=0.9))           # no factor
    with pytest.raises(ValueError):
        D.CUDAPrefetcher([], "cpu", synthesize_lr_bsrgan=dict(upscale_factor=4, noise=1))
    p = D.CUDAPrefetcher([], "cpu", synthesize_lr_bsrgan=dict(upscale_factor=4, jpeg_prob=0.5))
    assert p.synthesize_lr_bsrgan == dict(upscale_factor=4, jpeg_prob=0.5) and p.synthesize_lr is None
    assert D.CUDAPrefetcher([], "cpu").synthesize_lr_bsrgan is None
