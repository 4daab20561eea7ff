"""NIQE on the GPU (sr_gan_fd_amd/csrc/iqa.hip + the NIQE module) against what the reference's torch NIQE computed on the CPU,
recorded in tests/golden/niqe.npz by tests/golden/make_golden_niqe.py with a synthetic model (the published niqe_model.mat is not
in the tree; parity with it is unpinned).

Bounds, and why:
  luma plane       exact      the fixture has no pixel within 1e-3 of a rounding tie; fp32 evaluation order moves y*255 by ~1e-5
  half-size plane  atol 1e-12 on values in [0,1].  The reference's resize runs in float32 (its dtype test casts every input), so the
                              plane holds float32 values; the kernel reproduces the float32 roundings in the reference's order
  alpha            exact      the fixture has no table-search gap under 1e-9 relative; fp64 summation-order noise is ~1e-13
  other features   rtol 1e-9  sums of at most 9216 fp64 terms, table values from the same host lgamma
  score            rtol 1e-8  follows from cond * 1e-12 < 1e-8, asserted below (cond is about 19)
Measured on the MI355X, maxima over cases A-C: luma identical, half-size plane identical (0.0), every alpha identical, other features
4.5e-15 relative, scores 1.1e-15 relative."""
import os

import numpy as np
import pytest
import torch

from tests import niqe_oracle as NO

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return NO.load_cases(os.path.join(golden_dir, "niqe.npz"))


@pytest.fixture(scope="module")
def model_path(fixture, tmp_path_factory):
    """the synthetic model through the real loading path: savemat, then NIQE's loadmat"""
    from scipy.io import savemat
    path = str(tmp_path_factory.mktemp("niqe") / "niqe_model.mat")
    savemat(path, {"mu_prisparam": fixture[0], "cov_prisparam": fixture[1]})
    return path


def make(case, model_path):
    from sr_gan_fd_amd.image_quality_assessment import NIQE
    return NIQE(case["crop_border"], model_path, case["block"], case["block"])


def check_features(name, what, feat, want):
    alpha_equal = (feat[..., NO.ALPHA_COLUMNS] == want[..., NO.ALPHA_COLUMNS]).all()
    print(f"case {name} ({what}): alpha equal {alpha_equal}, features max rel {(np.abs(feat - want) / np.abs(want)).max():.2e}")
    assert feat.shape == want.shape
    assert alpha_equal
    np.testing.assert_allclose(feat, want, rtol=1e-9, atol=0)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_stages_and_score_match_reference(fixture, model_path, name):
    _, _, cond, cases = fixture
    c = cases[name]
    m = make(c, model_path)
    x = torch.from_numpy(c["input"]).to(DEV)
    feat, luma, half = m.features(x)
    score = m(x)
    assert score.shape == (x.shape[0],) and score.dtype == torch.float64 and score.is_cuda
    luma, half, feat, score = luma.cpu().numpy(), half.cpu().numpy(), feat.cpu().numpy(), score.cpu().numpy()
    err_half, err_score = np.abs(half - c["half"]).max(), np.abs(score / c["score"] - 1).max()
    print(f"case {name}: luma equal {(luma == c['luma']).all()}, half max abs {err_half:.2e}, score {score}, max rel {err_score:.2e}")
    assert luma.shape == c["luma"].shape and (luma == c["luma"]).all()
    assert half.shape == c["half"].shape and err_half <= 1e-12
    check_features(name, "from RGB", feat, c["feat"])
    assert cond * 1e-12 < 1e-8
    np.testing.assert_allclose(score, c["score"], rtol=1e-8, atol=0)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_features_from_luma_and_resize_entries(fixture, model_path, name):
    """the C entry points that start from the fp64 luma plane, and the half-size resize on its own"""
    from sr_gan_fd_amd import _abi as A
    c = fixture[3][name]
    m = make(c, model_path)
    table = m._on(DEV)[0]
    luma = torch.from_numpy(c["luma"]).to(DEV)
    n, h, w = luma.shape
    feat = torch.empty(n, c["feat"].shape[1], 36, dtype=torch.float64, device=DEV)
    half = torch.empty(n, h // 2, w // 2, dtype=torch.float64, device=DEV)
    A.check(A.lib().srganfd_niqe_features_luma(luma.data_ptr(), n, h, w, c["block"], c["block"], table.data_ptr(), table.shape[1], feat.data_ptr(),
                                               half.data_ptr(), A.stream_ptr()), "niqe_features_luma")
    check_features(name, "from the luma plane", feat.cpu().numpy(), c["feat"])
    assert np.abs(half.cpu().numpy() - c["half"]).max() <= 1e-12
    src = luma / 255.0
    alone = torch.empty_like(half)
    A.check(A.lib().srganfd_resize_half(src.data_ptr(), n, h, w, alone.data_ptr(), A.stream_ptr()), "resize_half")
    assert np.abs(alone.cpu().numpy() - c["half"]).max() <= 1e-12
    # odd sizes: ceil(h/2) x ceil(w/2), against the specification's restatement
    odd = src[:, :h - 1, :w - 3].contiguous()
    out = torch.empty(n, h // 2, (w - 2) // 2, dtype=torch.float64, device=DEV)
    A.check(A.lib().srganfd_resize_half(odd.data_ptr(), n, h - 1, w - 3, out.data_ptr(), A.stream_ptr()), "resize_half")
    assert np.abs(out.cpu().numpy() - NO.half_size(odd.cpu().numpy())).max() <= 1e-12


def test_deterministic_and_batch_independent(fixture, model_path):
    c = fixture[3]["A"]
    m = make(c, model_path)
    x = torch.from_numpy(c["input"]).to(DEV)
    first, again = m(x), m(x)
    assert torch.equal(first, again)
    singly = torch.cat([m(x[0:1]), m(x[1:2])])
    assert torch.equal(first, singly)
    f2, f1 = m.features(x)[0], torch.cat([m.features(x[0:1])[0], m.features(x[1:2])[0]])
    assert torch.equal(f2, f1)


def test_non_contiguous_and_half_precision_inputs(fixture, model_path):
    c = fixture[3]["A"]
    m = make(c, model_path)
    x = torch.from_numpy(c["input"]).to(DEV)
    nc = x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not nc.is_contiguous() and torch.equal(nc, x)
    assert torch.equal(m(nc), m(x))
    h = x.half()
    assert torch.equal(m(h), m(h.contiguous().float()))


def test_errors_name_the_problem(fixture, model_path, tmp_path):
    from scipy.io import savemat
    from sr_gan_fd_amd import _abi as A
    from sr_gan_fd_amd.image_quality_assessment import NIQE
    m = NIQE(4, model_path)
    with pytest.raises(A.SrganfdError, match="on the GPU"):
        m(torch.rand(1, 3, 200, 296))
    with pytest.raises(A.SrganfdError, match="3-channel"):
        m(torch.rand(1, 1, 200, 296, device=DEV))
    with pytest.raises(A.SrganfdError, match="at least 2"):
        m(torch.rand(1, 3, 104, 190, device=DEV))               # 96 x 182 after the crop: one block
    with pytest.raises(A.SrganfdError, match="larger than"):
        m(torch.rand(1, 3, 100, 296, device=DEV))
    with pytest.raises(A.SrganfdError, match="nowhere.mat"):
        NIQE(4, str(tmp_path / "nowhere.mat"))
    partial = str(tmp_path / "partial.mat")
    savemat(partial, {"mu_prisparam": fixture[0]})
    with pytest.raises(A.SrganfdError, match="cov_prisparam"):
        NIQE(4, partial)


def test_saturated_corner_is_finite_and_repeatable(model_path):
    """Robustness, no parity: a clamped SR output with one saturated, block-aligned 110 x 110 corner.  There is NO comparison with
    the reference here: on the constant block its MSCN values are rounding residue of about 1e-11 whose signs follow the summation
    order of its convolution, so its fitted shape jumps between the table ends (0.2 / 10) from one evaluation order to another (seen
    with the reference on the CPU).  The kernel's order is fixed, so its answer is repeatable; it must be finite."""
    from sr_gan_fd_amd.image_quality_assessment import NIQE
    g = torch.Generator().manual_seed(7)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, 296), torch.linspace(0, 1, 392), indexing="ij")
    x = (0.5 + 0.2 * torch.sin(9 * xx) * torch.cos(7 * yy) + 0.06 * torch.randn(2, 3, 296, 392, generator=g)).clamp(0, 1)
    x[:, :, :110, :110] = 1.0
    m = NIQE(4, model_path)
    x = x.to(DEV)
    a, b = m(x), m(x)
    feat = m.features(x)[0]
    assert torch.isfinite(a).all() and not torch.isnan(a).any()
    assert torch.equal(a, b)
    print("saturated corner: scores", a.cpu().numpy(), "NaN features", int(torch.isnan(feat).sum()))
