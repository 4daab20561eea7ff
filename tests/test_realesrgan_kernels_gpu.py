"""Real-ESRGAN's filter-kernel synthesis on the GPU (sr_gan_fd_amd/csrc/blur_kernels.hip through imgproc.blur_kernel_bank,
realesrgan_blur_kernels and the prefetcher's ``synthesize_kernels_realesrgan``) against the reference's recorded kernels
(tests/golden/realesrgan_kernels.npz).  Needs numpy and the fixture only.

Every comparison with the fixture is held to realesrgan_kernels_oracle.compare's bound, with ref32 = float32(reference):
    |out - ref32| <= np.spacing(|ref32|) + 1e-12 max|ref|
Both sides evaluate in fp64 and round once to float32, so the fp64 differences between them (the device's exp / pow / j1 against numpy's
and scipy's, a tree-shaped sum against numpy's pairwise one over at most 441 terms) can move a value across one float32 rounding boundary
and no further; the absolute term covers J1 near its zeros and values in float32's subnormal range.  The share of elements that are not
bit-equal is printed (DESIGN.md records it) and not gated."""
import os
import random

import numpy as np
import pytest
import torch

from tests import realesrgan_kernels_oracle as KO

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SIZES = list(range(7, 22, 2))


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return KO.load_fixture(os.path.join(golden_dir, "realesrgan_kernels.npz"))


def seed_all(s):
    random.seed(s)
    np.random.seed(s)


def bank(cases, kmax):
    from sr_gan_fd_amd.imgproc import blur_kernel_bank
    out = blur_kernel_bank([c["kind"] for c in cases], [c["ksize"] for c in cases], np.stack([c["params"] for c in cases]), kmax, DEV)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and out.shape == (len(cases), kmax, kmax) and out.device == DEV
    return out.cpu().numpy()


def check_against(out, cases, kmax, what):
    worst, unequal, total = -np.inf, 0, 0
    for i, c in enumerate(cases):
        excess, ne = KO.compare(out[i], KO.centred(c["ref"], kmax))
        assert excess <= 0, (what, i, c["family"], c["ksize"], list(c["params"]), excess)
        k, o = c["ksize"], (kmax - c["ksize"]) // 2
        pad = np.ones((kmax, kmax), dtype=bool)
        pad[o:o + k, o:o + k] = False
        assert (out[i][pad].view(np.uint32) == 0).all(), (what, i)                       # exactly +0.0f around the kernel
        assert abs(out[i].astype(np.float64).sum() - 1.0) <= 1e-5, (what, i)
        worst, unequal, total = max(worst, excess), unequal + ne, total + k * k
    print(f"{what}: {len(cases)} kernels, {unequal} of {total} elements not bit-equal to float32(reference) ({unequal / total:.2e})")
    return unequal, total


@pytest.mark.parametrize("kmax", [21, 25])
def test_sweep(fixture, kmax):
    cases = fixture["sweep"]
    check_against(bank(cases, kmax), cases, kmax, f"sweep, kmax {kmax}")


def test_sweep_without_padding(fixture):
    cases = [c for c in fixture["sweep"] if c["ksize"] == 7]
    assert len(cases) >= 14
    check_against(bank(cases, 7), cases, 7, "sweep, kmax = ksize = 7")


def test_single_kernel(fixture):
    for c in (fixture["sweep"][0], next(c for c in fixture["sweep"] if c["kind"] == 4 and c["ksize"] == 21)):
        check_against(bank([c], 21), [c], 21, "n = 1")


def mixed_bank(fixture):
    """all five kinds and all eight sizes in one launch: per size a Gaussian, a generalized, a plateau and a sinc kernel, deltas between"""
    cases = []
    for k in SIZES:
        for kind in (1, 2, 3, 4):
            cases.append([c for c in fixture["sweep"] if c["kind"] == kind and c["ksize"] == k][-1])
        cases.append({"family": "delta", "kind": 0, "ksize": k, "params": np.zeros(5)})
    return cases


def test_mixed_bank_deltas_and_identical_bits(fixture):
    cases = mixed_bank(fixture)
    assert {c["kind"] for c in cases} == {0, 1, 2, 3, 4} and {c["ksize"] for c in cases} == set(SIZES)
    out = bank(cases, 21)
    real = [i for i, c in enumerate(cases) if c["kind"]]
    check_against(out[real], [cases[i] for i in real], 21, "mixed bank")
    one = np.zeros((21, 21), dtype=np.float32)
    one[10, 10] = 1.0
    for i, c in enumerate(cases):
        if c["kind"] == 0:
            assert out[i].tobytes() == one.tobytes(), i                                  # exactly one 1.0f, +0.0f elsewhere, whatever ksize says
    assert bank(cases, 21).tobytes() == out.tobytes()                                    # a fixed-order reduction: the same bits again
    # a delta's ksize is ignored even where it would be refused for another kind
    odd = [dict(cases[4], ksize=k) for k in (0, 8, 99)]
    assert all(o.tobytes() == one.tobytes() for o in bank(odd, 21))


def test_seeded_batches(fixture):
    from sr_gan_fd_amd.imgproc import realesrgan_blur_kernels, realesrgan_kernel_draws
    unequal = total = 0
    for seed, case in fixture["seeds"].items():
        seed_all(seed)
        draws = realesrgan_kernel_draws(4, fixture["config"])
        got = realesrgan_blur_kernels(draws, fixture["config"], DEV)
        torch.cuda.synchronize()
        assert len(got) == 3
        for name, rec, t in zip(("gaussian_kernel1", "gaussian_kernel2", "sinc_kernel"), ("kernel1", "kernel2", "sinc_kernel"), got):
            want = case[name]
            assert t.dtype == torch.float32 and tuple(t.shape) == want.shape == (4, 21, 21) and t.device == DEV
            out = t.cpu().numpy()
            for n in range(4):
                excess, ne = KO.compare(out[n], want[n])
                assert excess <= 0, (seed, name, n, excess)
                k = draws[n][rec]["ksize"] if draws[n][rec]["kind"] else 1                # a delta: everything but the centre is padding
                pad = np.ones((21, 21), dtype=bool)
                pad[10 - k // 2:11 + k // 2, 10 - k // 2:11 + k // 2] = False
                assert (out[n][pad].view(np.uint32) == 0).all() and (want[n][pad] == 0).all(), (seed, name, n)
                unequal, total = unequal + ne, total + k * k
    print(f"seeded batches: {unequal} of {total} elements not bit-equal to the reference's float32 ({unequal / total:.2e})")


def test_two_kernel_sizes_take_two_launches(fixture):
    """sinc_kernel_size != gaussian_kernel_range[-1]: the blur kernels at one size, the sinc filters at the other"""
    from sr_gan_fd_amd.imgproc import realesrgan_blur_kernels
    seed = min(fixture["seeds"])
    case = fixture["seeds"][seed]
    k1, k2, k3 = realesrgan_blur_kernels(case["draws"], dict(fixture["config"], sinc_kernel_size=25), DEV)
    torch.cuda.synchronize()
    assert tuple(k1.shape) == tuple(k2.shape) == (4, 21, 21) and tuple(k3.shape) == (4, 25, 25)
    for n in range(4):
        assert KO.compare(k1[n].cpu().numpy(), case["gaussian_kernel1"][n])[0] <= 0 and KO.compare(k2[n].cpu().numpy(), case["gaussian_kernel2"][n])[0] <= 0
        assert KO.compare(k3[n].cpu().numpy(), KO.centred(case["sinc_kernel"][n], 25))[0] <= 0


def test_launch_on_another_stream_feeds_filter2d(fixture):
    from sr_gan_fd_amd.imgproc import blur_kernel_bank, filter2d_torch
    cases = [c for c in fixture["sweep"] if c["ksize"] == 13][:3]
    torch.manual_seed(0)
    image = torch.rand(3, 3, 40, 56, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        kernels = blur_kernel_bank([c["kind"] for c in cases], [c["ksize"] for c in cases], np.stack([c["params"] for c in cases]), 21, DEV)
    consumer = torch.cuda.current_stream(DEV)
    consumer.wait_stream(side)
    kernels.record_stream(consumer)
    got = filter2d_torch(image, kernels)
    want = filter2d_torch(image, torch.from_numpy(np.stack([KO.centred(c["ref"], 21) for c in cases]).astype(np.float32)).to(DEV))
    torch.cuda.synchronize()
    check_against(kernels.cpu().numpy(), cases, 21, "side stream")
    # positive taps that sum to 1, each within one spacing (<= 2^-23 relative) of float32(reference), on a [0, 1) image: the exact results
    # differ by <= 2^-23, and each run's fp32 accumulation of at most 441 taps is within 441 * 2^-25 of its exact result
    assert torch.isfinite(got).all() and (got - want).abs().max().item() <= 2.0 ** -23 + 2 * 441 * 2.0 ** -25


def test_prefetcher_adds_the_kernels(fixture):
    from sr_gan_fd_amd.dataset import CUDAPrefetcher
    P = fixture["config"]
    seed = min(fixture["seeds"])
    own = torch.rand(4, 21, 21)
    loader = [{"gt": torch.rand(4, 3, 32, 32)}, {"gt": torch.rand(2, 3, 32, 32)},
              {"gt": torch.rand(4, 3, 32, 32), "gaussian_kernel1": own, "gaussian_kernel2": own, "sinc_kernel": own}]
    seed_all(seed)
    pf = CUDAPrefetcher(loader, DEV, synthesize_kernels_realesrgan=P)
    first, second, third = pf.next(), pf.next(), pf.next()
    assert pf.next() is None
    torch.cuda.synchronize()
    for batch, b in ((first, 4), (second, 2)):
        assert set(batch) == {"gt", "gaussian_kernel1", "gaussian_kernel2", "sinc_kernel"}
        for name in ("gaussian_kernel1", "gaussian_kernel2", "sinc_kernel"):
            t = batch[name]
            assert t.dtype == torch.float32 and tuple(t.shape) == (b, 21, 21) and t.device == DEV
            assert ((t.double().sum(dim=(1, 2)) - 1).abs() <= 1e-5).all()
    # the first batch was staged right after the seeding: the fixture's batch
    for name in ("gaussian_kernel1", "gaussian_kernel2", "sinc_kernel"):
        for n in range(4):
            assert KO.compare(first[name][n].cpu().numpy(), fixture["seeds"][seed][name][n])[0] <= 0
        assert torch.equal(third[name].cpu(), own)                                       # a batch that brings its kernels keeps them
    plain = CUDAPrefetcher(loader[:1], DEV).next()
    assert set(plain) == {"gt"}                                                          # the default changes nothing


def test_degradation_process_takes_the_kernels(fixture):
    from sr_gan_fd_amd import imgproc
    from tests.test_oracle_golden import PIPE_PARAMS
    seed_all(5)
    torch.manual_seed(5)
    draws = imgproc.realesrgan_kernel_draws(2, fixture["config"])
    k1, k2, sinc = imgproc.realesrgan_blur_kernels(draws, fixture["config"], DEV)
    gt = torch.rand(2, 3, 64, 64, device=DEV)
    gt_usm, gt_out, lr = imgproc.degradation_process(gt, k1, k2, sinc, 4, PIPE_PARAMS, imgproc.DiffJPEG().to(DEV), imgproc.USMSharp().to(DEV))
    torch.cuda.synchronize()
    assert tuple(lr.shape) == (2, 3, 16, 16) and tuple(gt_usm.shape) == (2, 3, 64, 64) and gt_out is gt
    assert torch.isfinite(lr).all() and torch.isfinite(gt_usm).all() and 0.0 <= lr.min().item() and lr.max().item() <= 1.0


def test_library_refuses_bad_arguments():
    from sr_gan_fd_amd import _abi as A
    from sr_gan_fd_amd.imgproc import blur_kernel_bank
    p = [[1.0, 1.0, 0.0, 1.0, 1.0]] * 2
    for kind, ksize, kmax, names in (([1, 5], [7, 7], 21, "kind[1]"), ([-1, 1], [7, 7], 21, "kind[0]"), ([1, 2], [7, 8], 21, "ksize[1]"),
                                     ([4, 1], [23, 7], 21, "ksize[0]"), ([1, 1], [7, 1], 21, "ksize[1]"), ([1, 1], [7, 7], 20, "kmax"),
                                     ([1, 1], [7, 7], 27, "kmax")):
        with pytest.raises(A.SrganfdError) as e:
            blur_kernel_bank(kind, ksize, p, kmax, DEV)
        assert names in str(e.value), (names, str(e.value))
