"""LPIPS on the GPU (sr_gan_fd_amd/csrc/lpips.hip + the LPIPS module) against the torch-CPU restatement of the published
definition run in float64 (tests/lpips_oracle.py), with synthetic seeded weights loaded through ``load_state_dict`` (the
published alex.pth / torchvision weights are on none of the project's machines; parity with them is unpinned).

Bounds, and why:
  total and each s_k   relative 8 G, where G is the largest relative gap between the SAME oracle run in float32 (torch's fp32
                       ops: the reference's own arithmetic) and in float64, over the six values of that case.  The
                       reference's own rounding sets the scale; the factor 8 allows for the different accumulation order of
                       the MFMA tiles (fma chains of 32 terms, their sums added in K order; K up to 3456).  G is computed live on the CPU.
  tap maps (case B)    atol 2e-5 x the map's maximum: an fp32 dot product of K <= 3456 terms carries about sqrt(K) x 6e-8 =
                       3.5e-6 relative to the magnitude of its terms, per layer, and five layers follow each other; a wrong tap, a
                       transposed edge or a shifted pool moves values by the order of the maximum itself.
  head alone           rtol 1e-5 against the fp64 formula: at most 384 fp32 terms go into each per-pixel sum (sqrt(384) x 6e-8
                       = 1.2e-6, twice: the norms and the weighted difference) and at most 70 per-pixel values into each
                       spatial mean (5e-7); 1e-5 leaves a factor of about 3 and is 1000 times below any indexing mistake.
  identical inputs, slices, run-to-run   exact.

G on an x86-64 host, relative, largest over the six values (normalize False / True):
  case A 1.40e-06 / 7.77e-07    case B 1.27e-06 / 2.23e-07    case C 7.04e-07 / 2.43e-07
The kernel's summation order replayed on the CPU stays within 1.01 G on all six cases.  MI355X figures: not recorded yet (this
file was written without a GPU run; test_matches_oracle prints them, DESIGN.md 4a has the table to fill)."""
import warnings

import pytest
import torch

from tests import lpips_oracle as LO

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def model():
    from sr_gan_fd_amd.image_quality_assessment import LPIPS
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = LPIPS(net="alex")
    m.load_state_dict(LO.synthetic_state_dict())
    return m.to(DEV)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_matches_oracle(model, name, normalize):
    c = LO.case(name, normalize)
    n = c["sr"].shape[0]
    total, per = model(c["sr"].to(DEV), c["gt"].to(DEV), retPerLayer=True, normalize=normalize)
    assert total.shape == (n, 1, 1, 1) and total.dtype == torch.float32 and total.is_cuda and not total.requires_grad
    assert len(per) == 5 and all(p.shape == (n, 1, 1, 1) for p in per)
    plain = model(c["sr"].to(DEV), c["gt"].to(DEV), normalize=normalize)
    assert torch.equal(plain, total)
    if n == 1:
        assert isinstance(total.item(), float)              # validate() calls .item() on it
    got = [total.reshape(-1).double().cpu()] + [p.reshape(-1).double().cpu() for p in per]
    want = [c["want"][0]] + c["want"][1]
    errs = [((g - w).abs() / w.abs()).max().item() for g, w in zip(got, want)]
    print(f"case {name} normalize={normalize}: G {c['G']:.3e}, GPU rel err total {errs[0]:.3e}, per layer " + " ".join(f"{e:.2e}" for e in errs[1:])
          + f"  (largest {max(errs) / c['G']:.2f} G)")
    for what, e in zip(["total", "s1", "s2", "s3", "s4", "s5"], errs):
        assert e <= 8 * c["G"], (what, e, c["G"])


def test_tap_maps_case_b(model):
    """layer by layer, so that a failure names its layer: (2N, h, w, C) NHWC maps, in0's images first"""
    c = LO.case("B")
    maps = model.features(c["sr"].to(DEV), c["gt"].to(DEV))
    want0, want1 = c["want"][2], c["want"][3]
    assert [tuple(m.shape[1:3]) for m in maps] == [(16, 21), (7, 10), (3, 4), (3, 4), (3, 4)]
    for k, m in enumerate(maps):
        want = torch.cat([want0[k], want1[k]]).permute(0, 2, 3, 1)
        got = m.double().cpu()
        assert got.shape == want.shape
        err = (got - want).abs().max().item()
        print(f"tap {k + 1}: max {want.max().item():.3f}, max abs err {err:.2e} ({err / want.max().item():.2e} of the max)")
        assert err <= 2e-5 * want.max().item(), k + 1
        assert ((got == 0) == (want == 0)).double().mean().item() > 0.999      # ReLU zeroes the same places (but for values at rounding distance from 0)


def test_padding_is_applied_after_scaling(model):
    """an all-zero image: the scaling layer turns it into -shift / scale everywhere INSIDE the image, and the first conv's
    padding stays 0.  Padding before the scaling would add about shift / scale times the border weights to tap 1's border."""
    sd = LO.synthetic_state_dict()
    z = torch.zeros(1, 3, 67, 90)
    want = LO.taps(z, sd, torch.float64)[0].permute(0, 2, 3, 1)
    got = model.features(z.to(DEV), z.to(DEV))[0].double().cpu()
    assert torch.equal(got[0], got[1])
    # what the wrong order would give: the padding ring holds the scaled constant too (a replicated border)
    x = (z.double() - sd["scaling_layer.shift"].double()) / sd["scaling_layer.scale"].double()
    wrong = torch.relu(torch.nn.functional.conv2d(torch.nn.functional.pad(x, (2, 2, 2, 2), mode="replicate"), sd["net.slice1.0.weight"].double(),
                                                  sd["net.slice1.0.bias"].double(), stride=4)).permute(0, 2, 3, 1)
    border = torch.ones(16, 21, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    assert (wrong[0][border] - want[0][border]).abs().max().item() > 1e-2          # the two orders are far apart on the border
    assert (got[0] - want[0]).abs().max().item() <= 2e-5 * want.max().item()


def test_identical_inputs_give_zero(model):
    x = LO.case("B")["gt"].to(DEV)
    total, per = model(x, x.clone(), retPerLayer=True)
    assert (total == 0).all() and all((p == 0).all() for p in per)


def test_slices_equal_their_contiguous_copies(model):
    """test_bsrgan.py:232-271 passes sr_tensor[:, :, a:b, c:d] slices"""
    c = LO.case("C")
    sr, gt = c["sr"].to(DEV), c["gt"].to(DEV)
    a, b = sr[:, :, 5:101, 17:150], gt[:, :, 5:101, 17:150]
    assert not a.is_contiguous()
    got = model(a, b)
    ref = model(a.contiguous(), b.contiguous())
    assert torch.equal(got, ref) and (got > 0).all()
    # a channels-last view: unit stride on the channel axis
    p = sr.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not p.is_contiguous() and torch.equal(model(p, gt), model(sr, gt))


def test_run_to_run_bit_equal(model):
    c = LO.case("C")
    sr, gt = c["sr"].to(DEV), c["gt"].to(DEV)
    first = model(sr, gt).clone()
    for _ in range(3):
        assert torch.equal(model(sr, gt), first)


@pytest.mark.parametrize("c,h,w", [(64, 1, 1), (64, 7, 10), (384, 1, 1), (384, 7, 10)])
def test_head_entry_point(c, h, w):
    """srganfd_lpips_head on synthetic maps; pixels that are all-zero vectors in one image, in both, and in neither"""
    from sr_gan_fd_amd import _abi as A
    n = 3
    g = torch.Generator().manual_seed(7 + c + h)
    maps = torch.relu(torch.randn(2 * n, h, w, c, generator=g))
    lin = torch.rand(c, generator=g) / c
    if h * w > 1:
        maps[0, 0, 0] = 0                       # zero in the first input only
        maps[n + 0, 1, 1] = 0                   # zero in the second input only
        maps[0, 2, 2] = 0
        maps[n + 0, 2, 2] = 0                   # zero in both
    else:
        maps[1] = 0                             # image 1: zero in the first input only (image 0: in neither)
        maps[2] = 0
        maps[n + 2] = 0                         # image 2: zero in both, the distance is exactly 0
    f0, f1 = maps[:n].double(), maps[n:].double()
    n0 = f0 / (f0.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    n1 = f1 / (f1.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    want = (((n0 - n1) ** 2) * lin.double()).sum(-1).mean(dim=(1, 2))
    md, ld = maps.to(DEV), lin.to(DEV)
    out = torch.full((2, n), float("nan"), device=DEV)
    ws = torch.empty(n * h * w, device=DEV)
    tap = (A.LpipsTap * 1)()
    tap[0].maps, tap[0].lin, tap[0].h, tap[0].w, tap[0].c = md.data_ptr(), ld.data_ptr(), h, w, c
    A.check(A.lib().srganfd_lpips_head(tap, 1, n, out.data_ptr(), ws.data_ptr(), A.stream_ptr()), "lpips_head")
    got = out.double().cpu()
    assert torch.isfinite(got).all()
    print(f"head C={c} {h}x{w}: want {want.tolist()}, max rel err {((got[0] - want).abs() / want.clamp_min(1e-30)).max().item():.2e}")
    assert torch.allclose(got[0], want, rtol=1e-5, atol=0)
    assert torch.equal(got[1], got[0])          # one tap: the total is that tap
