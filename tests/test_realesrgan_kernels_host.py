"""The host side of Real-ESRGAN's filter-kernel synthesis (sr_gan_fd_amd/imgproc.py: realesrgan_kernel_draws, the parameter-dict check, the
argument checks of blur_kernel_bank / realesrgan_blur_kernels / CUDAPrefetcher, and srganfd_blur_kernel_bank's own validation in dry-run
mode) against tests/golden/realesrgan_kernels.npz (tests/golden/make_golden_realesrgan_kernels.py: the reference's dataset run on seeded
streams).  No GPU."""
import copy
import os
import random

import numpy as np
import pytest
import torch

from tests import realesrgan_kernels_oracle as KO


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return KO.load_fixture(os.path.join(golden_dir, "realesrgan_kernels.npz"))


def seed_all(s):
    random.seed(s)
    np.random.seed(s)


def test_fixture_covers_the_cases(fixture):
    sweep = fixture["sweep"]
    assert {c["family"] for c in sweep} == {"isotropic", "anisotropic", "generalized_isotropic", "generalized_anisotropic", "plateau_isotropic",
                                            "plateau_anisotropic", "sinc"}
    for family in {c["family"] for c in sweep}:
        assert {c["ksize"] for c in sweep if c["family"] == family} == set(range(7, 22, 2)), family
    P = np.stack([c["params"] for c in sweep])
    kind = np.array([c["kind"] for c in sweep])
    assert {0.2, 3.0} <= set(P[:, 0]) and (P[kind < 4, 0] != P[kind < 4, 1]).any()
    assert {-np.pi, 0.7, np.pi} <= set(P[:, 2])
    assert set(P[kind == 2, 3]) == {0.5, 1.0, 4.0} and set(P[kind == 3, 3]) == {1.0, 2.0}
    assert set(P[kind == 4, 4]) == {np.pi / 5, np.pi / 3, np.pi}
    assert len(fixture["seeds"]) == 2
    for case in fixture["seeds"].values():
        recs = [r[n] for r in case["draws"] for n in ("kernel1", "kernel2")]
        assert len(case["draws"]) == 4 and any(r["kernel1"]["kind"] == 4 for r in case["draws"])
        assert {r["sinc_kernel"]["kind"] for r in case["draws"]} == {0, 4} and {2, 3} <= {r["kind"] for r in recs}


def test_draws_follow_the_reference_streams(fixture):
    from sr_gan_fd_amd.imgproc import realesrgan_kernel_draws
    for seed, case in fixture["seeds"].items():
        seed_all(seed)
        draws = realesrgan_kernel_draws(4, fixture["config"])
        assert draws == case["draws"], seed
        assert random.random() == case["end"][0] and np.random.rand() == case["end"][1], seed        # both streams where the reference left them
        for rec in draws:
            assert set(rec) == {"kernel1", "kernel2", "sinc_kernel"}
            for r in rec.values():
                assert set(r) == {"kind", "ksize", "sigma_x", "sigma_y", "theta", "beta", "omega"}
                assert type(r["kind"]) is int and type(r["ksize"]) is int and all(type(r[f]) is float for f in ("sigma_x", "sigma_y", "theta", "beta", "omega"))
                if r["kind"] in (1, 2, 3) and r["theta"] == 0.0:
                    assert r["sigma_y"] == r["sigma_x"]


def test_draws_branches(fixture):
    """probabilities 0 / 1 force each branch; the draws stay inside the configured ranges; an unknown type name is the isotropic Gaussian"""
    from sr_gan_fd_amd.imgproc import realesrgan_kernel_draws
    P = copy.deepcopy(fixture["config"])
    P.update(sinc_kernel_probability1=1.0, sinc_kernel_probability2=0.0, sinc_kernel_probability3=0.0, gaussian_kernel_type=["no_such_kernel"],
             gaussian_kernel_probability2=[1.0])
    P["gaussian_kernel_probability1"] = [1.0]
    seed_all(3)
    for rec in realesrgan_kernel_draws(16, P):
        k1, k2, k3 = rec["kernel1"], rec["kernel2"], rec["sinc_kernel"]
        assert k1["kind"] == 4 and (np.pi / 3 if k1["ksize"] < 14 else np.pi / 5) <= k1["omega"] <= np.pi and k1["ksize"] in P["gaussian_kernel_range"]
        assert k2["kind"] == 1 and k2["sigma_y"] == k2["sigma_x"] and k2["theta"] == 0.0 and 0.2 <= k2["sigma_x"] <= 1.5
        assert k3 == {"kind": 0, "ksize": 21, "sigma_x": 0.0, "sigma_y": 0.0, "theta": 0.0, "beta": 0.0, "omega": 0.0}
    P.update(gaussian_kernel_type=["plateau_anisotropic", "generalized_isotropic"], sinc_kernel_probability1=0.0, sinc_kernel_probability3=1.0)
    P["gaussian_kernel_probability1"], P["gaussian_kernel_probability2"] = [1.0, 0.0], [0.0, 1.0]
    seed_all(4)
    for rec in realesrgan_kernel_draws(16, P):
        k1, k2, k3 = rec["kernel1"], rec["kernel2"], rec["sinc_kernel"]
        assert k1["kind"] == 3 and 1.0 <= k1["beta"] <= 2.0 and 0.2 <= k1["sigma_y"] <= 3.0 and -np.pi <= k1["theta"] <= np.pi
        assert k2["kind"] == 2 and 0.5 <= k2["beta"] <= 4.0 and k2["sigma_y"] == k2["sigma_x"]
        assert k3["kind"] == 4 and np.pi / 3 <= k3["omega"] <= np.pi


def test_parameter_dict_validation(fixture):
    from sr_gan_fd_amd.imgproc import check_realesrgan_kernel_parameters, realesrgan_blur_kernels, realesrgan_kernel_draws
    good = fixture["config"]
    check_realesrgan_kernel_parameters(good)
    for key in good:
        P = {k: v for k, v in good.items() if k != key}
        for call in (lambda: check_realesrgan_kernel_parameters(P), lambda: realesrgan_kernel_draws(1, P), lambda: realesrgan_blur_kernels([], P)):
            with pytest.raises(ValueError, match=key):
                call()
    for key, bad in (("gaussian_kernel_range", [7, 8]), ("gaussian_kernel_range", [7, 27]), ("gaussian_kernel_range", [21, 7]),
                     ("gaussian_kernel_range", []), ("sinc_kernel_size", 20), ("sinc_kernel_size", 27), ("sinc_kernel_size", 21.0),
                     ("gaussian_kernel_probability1", [1.0]), ("gaussian_kernel_type", []), ("gaussian_sigma_range2", [1.5, 0.2]),
                     ("gaussian_sigma_range1", [1.0]), ("plateau_kernel_beta_range2", [1, 2, 3])):
        with pytest.raises(ValueError, match=key):
            check_realesrgan_kernel_parameters(dict(good, **{key: bad}))
    with pytest.raises(ValueError):
        check_realesrgan_kernel_parameters(None)
    # a drawn sinc filter that does not fit sinc_kernel_size is refused before anything is launched
    draws = copy.deepcopy(fixture["seeds"][min(fixture["seeds"])]["draws"])
    n = next(i for i, r in enumerate(draws) if r["sinc_kernel"]["kind"] == 4)
    draws[n]["sinc_kernel"]["ksize"] = 21
    with pytest.raises(ValueError, match=f"image {n}"):
        realesrgan_blur_kernels(draws, dict(good, sinc_kernel_size=19))


def test_blur_kernel_bank_argument_checks():
    from sr_gan_fd_amd import _abi as A
    from sr_gan_fd_amd.imgproc import blur_kernel_bank
    p = [[1.0, 1.0, 0.0, 1.0, 1.0]]
    for kind, ksize, params, kmax in (([], [], np.zeros((0, 5)), 21), ([1, 1], [7], p * 2, 21), ([1], [7], [[1.0] * 4], 21), ([1], [7], p * 2, 21),
                                      ([1.0], [7], p, 21), ([1], [7.0], p, 21), ([[1]], [[7]], p, 21), ([1], [7], [["a"] * 5], 21),
                                      ([1], [7], p, 21.0), ([1], [7], p, None)):
        with pytest.raises(A.SrganfdError):
            blur_kernel_bank(kind, ksize, params, kmax)
    with pytest.raises(A.SrganfdError, match="GPU"):
        blur_kernel_bank([1], [7], p, 21, device="cpu")                # the HIP library is the product: no CPU path


def test_library_validation_dry_run():
    """srganfd_blur_kernel_bank validates before it launches, so every refusal shows without a GPU"""
    from sr_gan_fd_amd import _abi as A
    L = A.lib()
    assert A.ABI_VERSION == 7 and L.srganfd_abi_version() == 7
    A.set_dry_run(True)
    try:
        kind, ksize = np.array([1, 4, 0], dtype=np.int32), np.array([7, 21, 0], dtype=np.int32)
        params, out = np.ones((3, 5)), np.zeros((3, 21, 21), dtype=np.float32)
        bank = lambda kd, ks, pr, kdh, ksh, n, kmax, o: L.srganfd_blur_kernel_bank(kd, ks, pr, kdh, ksh, n, kmax, o, 0)
        ptr = lambda a: a.ctypes.data
        assert bank(ptr(kind), ptr(ksize), ptr(params), ptr(kind), ptr(ksize), 3, 21, ptr(out)) == 0      # a delta's size is ignored
        assert bank(ptr(kind), ptr(ksize), ptr(params), None, None, 3, 21, ptr(out)) == 0
        for hole in range(3):
            args = [ptr(kind), ptr(ksize), ptr(params)]
            args[hole] = None
            assert bank(*args, ptr(kind), ptr(ksize), 3, 21, ptr(out)) == -1
        assert bank(ptr(kind), ptr(ksize), ptr(params), ptr(kind), ptr(ksize), 3, 21, None) == -1
        assert bank(ptr(kind), ptr(ksize), ptr(params), ptr(kind), None, 3, 21, ptr(out)) == -1            # one host array without the other
        assert bank(ptr(kind), ptr(ksize), ptr(params), None, ptr(ksize), 3, 21, ptr(out)) == -1
        for n in (0, -1):
            assert bank(ptr(kind), ptr(ksize), ptr(params), ptr(kind), ptr(ksize), n, 21, ptr(out)) == -1
        for kmax in (1, 20, 27, -3):
            assert bank(ptr(kind), ptr(ksize), ptr(params), None, None, 3, kmax, ptr(out)) == -1
            assert "kmax" in L.srganfd_last_error().decode()
        for bad in (5, -1):
            kb = np.array([1, bad, 0], dtype=np.int32)
            assert bank(ptr(kb), ptr(ksize), ptr(params), ptr(kb), ptr(ksize), 3, 21, ptr(out)) == -1
            assert "kind[1]" in L.srganfd_last_error().decode()
        for bad in (8, 23, 1, 0, -7):
            sb = np.array([7, 21, bad], dtype=np.int32)
            k3 = np.array([1, 4, 3], dtype=np.int32)
            assert bank(ptr(k3), ptr(sb), ptr(params), ptr(k3), ptr(sb), 3, 21, ptr(out)) == -1
            assert "ksize[2]" in L.srganfd_last_error().decode()
        s25 = np.array([7, 25, 0], dtype=np.int32)
        out25 = np.zeros((3, 25, 25), dtype=np.float32)
        assert bank(ptr(kind), ptr(s25), ptr(params), ptr(kind), ptr(s25), 3, 25, ptr(out25)) == 0
    finally:
        A.set_dry_run(False)


def test_prefetcher_argument_checks(monkeypatch, fixture):
    from sr_gan_fd_amd import dataset as D

    class Stream:
        def __init__(self, device=None):
            pass

    monkeypatch.setattr(torch.cuda, "Stream", Stream)
    monkeypatch.setattr(D.CUDAPrefetcher, "reset", lambda self: None)                  # no batch is staged: only the constructor runs
    good = fixture["config"]
    for key in good:
        with pytest.raises(ValueError, match=key):
            D.CUDAPrefetcher([], "cpu", synthesize_kernels_realesrgan={k: v for k, v in good.items() if k != key})
    with pytest.raises(ValueError, match="sinc_kernel_size"):
        D.CUDAPrefetcher([], "cpu", synthesize_kernels_realesrgan=dict(good, sinc_kernel_size=20))
    with pytest.raises(ValueError):
        D.CUDAPrefetcher([], "cpu", synthesize_kernels_realesrgan=21)
    p = D.CUDAPrefetcher([], "cpu", synthesize_kernels_realesrgan=good)
    assert p.synthesize_kernels_realesrgan == good and p.synthesize_kernels_realesrgan is not good
    assert D.CUDAPrefetcher([], "cpu").synthesize_kernels_realesrgan is None
