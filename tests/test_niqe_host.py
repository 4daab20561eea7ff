"""CPU-only NIQE tests: the numpy restatement of the specification (tests/niqe_oracle.py) reproduces every case of
tests/golden/niqe.npz within the bounds the GPU tests use; the new C entry points are declared, bound and exported; their argument
validation answers in dry-run mode, where nothing is launched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import niqe_oracle as NO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("srganfd_niqe_workspace_doubles", "srganfd_niqe_features", "srganfd_niqe_features_luma", "srganfd_resize_half")


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return NO.load_cases(os.path.join(golden_dir, "niqe.npz"))


def test_fixture_conditioning(fixture):
    """the score tolerance 1e-8 follows from the conditioning of the averaged covariance: cond * 1e-12 < 1e-8"""
    assert fixture[2] * 1e-12 < 1e-8


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_oracle_reproduces_reference(fixture, name):
    """Measured here (maxima over the three cases): luma and half-size planes identical, every alpha identical, other features
    2.9e-12 relative, scores 8.9e-16 relative."""
    mu, cov, _, cases = fixture
    c = cases[name]
    score, luma, half, feat = NO.niqe(c["input"], c["crop_border"], mu, cov, c["block"], c["block"])
    assert luma.shape == c["luma"].shape and (luma == c["luma"]).all()
    err_half = np.abs(half - c["half"]).max()
    alpha_equal = (feat[..., NO.ALPHA_COLUMNS] == c["feat"][..., NO.ALPHA_COLUMNS]).all()
    err_feat = (np.abs(feat - c["feat"]) / np.abs(c["feat"])).max()
    err_score = np.abs(score / c["score"] - 1).max()
    print(f"case {name}: half max abs {err_half:.2e}, alpha equal {alpha_equal}, features max rel {err_feat:.2e}, score max rel {err_score:.2e}")
    assert err_half <= 1e-12
    assert alpha_equal
    np.testing.assert_allclose(feat, c["feat"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(score, c["score"], rtol=1e-8, atol=0)


def test_features_from_the_fixture_luma(fixture):
    """the second entry of the specification: features from the recorded luma plane alone"""
    c = fixture[3]["C"]
    feat, half = NO.features(c["luma"], c["block"], c["block"])
    assert (half == c["half"]).all()
    np.testing.assert_allclose(feat, c["feat"], rtol=1e-9, atol=0)


def test_block_order_is_column_major(fixture):
    """a (N, blocks, 36) matrix written row-major would not match case B (4 x 3 blocks): feature rows differ between blocks"""
    c = fixture[3]["B"]
    feat, _ = NO.features(c["luma"], c["block"], c["block"])
    nby, nbx = c["luma"].shape[1] // c["block"], c["luma"].shape[2] // c["block"]
    assert (nby, nbx) == (4, 3)
    row_major = feat.reshape(1, nbx, nby, 36).transpose(0, 2, 1, 3).reshape(1, -1, 36)
    assert not np.allclose(row_major, c["feat"], rtol=1e-3)


def test_half_taps_are_dyadic():
    """the kernel hard-codes the ten weights; they are exact in float32"""
    want = [0.0, -0.01171875, -0.03515625, 0.11328125, 0.43359375, 0.43359375, 0.11328125, -0.03515625, -0.01171875, 0.0]
    assert NO.half_taps().tolist() == want and NO.half_taps().astype(np.float32).astype(np.float64).tolist() == want


def test_new_symbols_declared_bound_exported():
    from sr_gan_fd_amd import _abi as A
    hdr = open(os.path.join(ROOT, "include", "srganfd.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", A.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in NEW_SYMBOLS:
        assert name in A.SYMBOLS, f"{name} missing from _abi.SYMBOLS"
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} not declared in include/srganfd.h"
        assert name in exported, f"{name} not exported by {A.LIB_PATH}"
    assert A.lib().srganfd_abi_version() == 7


def test_package_imports_niqe_without_touching_scipy():
    """scipy is needed by NIQE's constructor only"""
    code = "import sys; from sr_gan_fd_amd.image_quality_assessment import PSNR, SSIM, NIQE; assert 'scipy' not in sys.modules"
    subprocess.run([os.sys.executable, "-c", code], check=True, cwd=ROOT)


def test_argument_validation_dry_run():
    from sr_gan_fd_amd import _abi as A
    L = A.lib()
    A.set_dry_run(True)
    try:
        p = 4096                                            # a non-null address; nothing is dereferenced in dry-run mode

        def err():
            return L.srganfd_last_error().decode()

        assert L.srganfd_niqe_workspace_doubles(2, 3, 200, 296, 4, 96, 96) == 2 * 192 * 288 + 2 * 96 * 144
        assert L.srganfd_niqe_features(p, 2, 3, 200, 296, 4, 96, 96, p, 9801, p, p, 0) == 0
        assert L.srganfd_niqe_features_luma(p, 2, 192, 288, 96, 96, p, 9801, p, p, 0) == 0
        assert L.srganfd_resize_half(p, 2, 192, 288, p, 0) == 0
        assert L.srganfd_resize_half(p, 1, 5, 7, p, 0) == 0
        # each bad argument: the query answers -1, the entry SRGANFD_EINVAL (-1), and the message names the problem
        for args, word in (((2, 1, 200, 296, 4, 96, 96), "3-channel"),          # c != 3
                           ((2, 3, 200, 296, 4, 95, 96), "even"),                 # odd block
                           ((2, 3, 100, 296, 4, 96, 96), "larger than"),          # block larger than the cropped image
                           ((2, 3, 104, 190, 4, 96, 96), "at least 2"),           # one block per image
                           ((2, 3, 400, 400, 0, 128, 128), "LDS"),                # 128 x 128 fp64 block + map exceed 160 KB
                           ((2, 3, 200, 296, -1, 96, 96), "crop_border")):
            assert L.srganfd_niqe_workspace_doubles(*args) == -1 and word in err(), (args, err())
            n, c, h, w, cb, bh, bw = args
            assert L.srganfd_niqe_features(p, n, c, h, w, cb, bh, bw, p, 9801, p, p, 0) == -1 and word in err(), (args, err())
        assert L.srganfd_niqe_features(None, 2, 3, 200, 296, 4, 96, 96, p, 9801, p, p, 0) == -1 and "null" in err()
        assert L.srganfd_niqe_features_luma(p, 2, 200, 288, 96, 96, p, 9801, p, p, 0) == -1 and "whole number" in err()
        assert L.srganfd_niqe_features_luma(p, 2, 96, 96, 96, 96, p, 9801, p, p, 0) == -1 and "at least 2" in err()
        assert L.srganfd_niqe_features_luma(p, 2, 192, 288, 96, 96, p, 1, p, p, 0) == -1 and "table" in err()
        assert L.srganfd_resize_half(p, 1, 3, 64, p, 0) == -1 and "resize_half" in err()
        assert L.srganfd_resize_half(None, 1, 64, 64, p, 0) == -1
    finally:
        A.set_dry_run(False)


def test_module_errors_without_gpu(tmp_path):
    """constructor and input errors need no GPU: a missing file, a file without cov_prisparam, a CPU tensor"""
    import torch
    from scipy.io import savemat
    from sr_gan_fd_amd import _abi as A
    from sr_gan_fd_amd.image_quality_assessment import NIQE
    missing = str(tmp_path / "nowhere.mat")
    with pytest.raises(A.SrganfdError, match="nowhere.mat"):
        NIQE(4, missing)
    partial = str(tmp_path / "partial.mat")
    savemat(partial, {"mu_prisparam": np.zeros((1, 36))})
    with pytest.raises(A.SrganfdError, match="cov_prisparam"):
        NIQE(4, partial)
    good = str(tmp_path / "good.mat")
    savemat(good, {"mu_prisparam": np.zeros((1, 36)), "cov_prisparam": np.eye(36)})
    with pytest.raises(A.SrganfdError, match="on the GPU"):
        NIQE(4, good)(torch.rand(1, 3, 200, 296))


def test_score_step_on_the_host(fixture, tmp_path):
    """the 36 x 36 step is plain torch and runs anywhere: recorded features -> recorded scores, through the symmetric eigensolver
    (symmetric model covariance, the usual case) and through the general SVD (a covariance off symmetry by one float32 step in one
    entry: that is another model, 1e-7 away, so its scores are compared at 1e-6)"""
    import torch
    from scipy.io import savemat
    from sr_gan_fd_amd.image_quality_assessment import NIQE
    mu, cov, _, cases = fixture
    skew = cov.copy()
    skew[3, 5] = np.nextafter(np.float32(skew[3, 5]), np.float32(np.inf))
    for name, matrix, symmetric in (("sym.mat", cov, True), ("skew.mat", skew, False)):
        path = str(tmp_path / name)
        savemat(path, {"mu_prisparam": mu, "cov_prisparam": matrix})
        m = NIQE(4, path)
        assert m._symmetric is symmetric
        for c in cases.values():
            np.testing.assert_allclose(m.score(torch.from_numpy(c["feat"])).numpy(), c["score"], rtol=1e-8 if symmetric else 1e-6, atol=0)
    # a block with a NaN feature leaves the covariance and its own column means; the score stays finite
    feat = torch.from_numpy(cases["A"]["feat"]).clone()
    feat[0, 2, 5] = float("nan")
    s = NIQE(4, str(tmp_path / "sym.mat")).score(feat)
    assert torch.isfinite(s).all() and s[1].item() == pytest.approx(cases["A"]["score"][1], rel=1e-8)
