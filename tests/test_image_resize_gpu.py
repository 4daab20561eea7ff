"""imgproc.image_resize on the GPU (sr_gan_fd_amd/csrc/imresize.hip) against the reference's recorded outputs
(tests/golden/image_resize.npz) and against the fp64-accumulating oracle of tests/resize_oracle.py, and the prefetcher's
``synthesize_lr``.

The bound is derived, not measured (tests/resize_oracle.py): B = 2 * (P + 3) * 2^-24 * S^2 for inputs in [0, 1], computed from the
case's tables.  Kernel vs oracle: <= B.  Kernel vs the reference's recorded float32 output: <= 2 B (both lie within B of the same
exact value).  This host's torch may round float32 ``**`` differently from the one that recorded the fixture, so the tests do not
assume that two table builders agree here: they measure delta = max |w_package - w_other| over the case's tables, print it, assert
delta <= 2^-20 (one unit in the last place of the cubic's largest intermediate, 8) and widen the bound by 2 * P * S * delta (each
pass moves by at most P * delta * M on values of magnitude M <= S).  delta is expected to be 0, which leaves B.
No case is skipped and no pixel is excluded.
Measured on the MI355X (every delta 0): kernel vs oracle at most 0.097 B over the fixture cases (x4) and 0.131 B over the training
shapes (x8); kernel vs the recorded reference at most 0.082 B of the allowed 2 B; NIQE's half-size planes 0.082 B."""
import math
import os

import numpy as np
import pytest
import torch

from tests import niqe_oracle as NO
from tests import resize_oracle as RO

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DELTA_MAX = 2.0 ** -20


@pytest.fixture(scope="module")
def cases(golden_dir):
    return RO.load_cases(os.path.join(golden_dir, "image_resize.npz"))


def resize(x, scale, aa=True):
    from sr_gan_fd_amd.imgproc import image_resize
    y = image_resize(x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).to(DEV), scale, aa)
    torch.cuda.synchronize()
    return y


def package_tables(h, w, scale, aa):
    from sr_gan_fd_amd.imgproc import _resize_tables_host
    out = []
    for n in (h, w):
        t = _resize_tables_host(n, math.ceil(n * scale), scale, aa)
        out.append((t[0].numpy(), t[1].numpy().astype(np.int64)))
    return out


def bounds(h, w, scale, aa, others=None):
    """(B, widening, delta): B, P and S from the oracle's tables; delta between the package's tables and `others` (default: the oracle's)"""
    mine = package_tables(h, w, scale, aa)
    orc = [RO.tables(n, math.ceil(n * scale), scale, aa) for n in (h, w)]
    others = orc if others is None else others
    delta = max(RO.table_delta(m[0], m[1], o[0], np.asarray(o[1], dtype=np.int64)) for m, o in zip(mine, others))
    p = max(t[0].shape[1] for t in orc)
    s = max(float(np.abs(t[0].astype(np.float64)).sum(1).max()) for t in orc)
    return RO.bound(orc[0][0], orc[1][0]), 2 * p * s * delta, delta


def check_vs_oracle(what, x, got, scale, aa=True):
    """x: numpy input in [0, 1], got: the kernel's output (tensor)"""
    h, w = x.shape[-2:]
    b, widen, delta = bounds(h, w, scale, aa)
    want = RO.resize(x, scale, aa)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == want.shape, (what, got.shape, want.shape)
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    print(f"{what}: kernel vs oracle {err:.3e} = {err / b:.3f} B (B {b:.3e}, table delta {delta:.1e})")
    assert delta <= DELTA_MAX
    assert err <= b + widen
    return err / b


def u8_grid(rng, *shape):
    return rng.randint(0, 256, size=shape).astype(np.uint8).astype(np.float32) / np.float32(255)


@pytest.mark.parametrize("name", RO.CASE_NAMES)
def test_fixture_case(cases, name):
    c = cases[name]
    x, scale, aa = c["input"], c["scale"], c["antialiasing"]
    h, w = x.shape[-2:]
    got = resize(x, scale, aa)
    assert got.dim() == x.ndim                                     # (C, H, W) in, (C, h, w) out; (H, W) in, (h, w) out
    check_vs_oracle(f"case {name}", x, got, scale, aa)
    recorded = [(c["weights_h"], c["first_h"]), (c["weights_w"], c["first_w"])]
    b, widen, delta = bounds(h, w, scale, aa, recorded)
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - c["output"].astype(np.float64)).max())
    print(f"case {name}: kernel vs recorded reference {err:.3e} = {err / b:.3f} B (table delta vs recorded {delta:.1e})")
    assert got.shape == c["output"].shape
    assert delta <= DELTA_MAX
    assert err <= 2 * b + widen


def test_forms_and_views(cases):
    """(H, W), (C, H, W) and (N, C, H, W) carry the same planes through the same tiles: identical bits; so does a non-contiguous view"""
    c = cases["q97x131"]
    x = torch.from_numpy(c["input"]).to(DEV)                       # (3, 97, 131)
    y3 = resize(x, c["scale"])
    y2 = resize(x[1], c["scale"])
    x4 = torch.stack([x, x.flip(0)])
    y4 = resize(x4, c["scale"])
    assert y3.shape == (3, 25, 33) and y2.shape == (25, 33) and y4.shape == (2, 3, 25, 33)
    assert torch.equal(y2, y3[1]) and torch.equal(y4[0], y3) and torch.equal(y4[1], y3.flip(0))
    big = torch.zeros(3, 120, 160, device=DEV)
    big[:, 11:108, 7:138] = x
    view = big[:, 11:108, 7:138]
    assert not view.is_contiguous() and torch.equal(resize(view, c["scale"]), y3)
    tr = x.transpose(1, 2).contiguous().transpose(1, 2)            # the same values, column-major in memory
    assert not tr.is_contiguous() and torch.equal(resize(tr, c["scale"]), y3)
    check_vs_oracle("batched form", x4.cpu().numpy(), y4, c["scale"])
    # other dtypes are converted to float32 first, as the reference's .float() does
    assert torch.equal(resize(x.double(), c["scale"]), y3)


@pytest.mark.parametrize("shape,scale,aa", [
    ((16, 3, 128, 128), 1 / 4, True),        # ESRGAN's training crop (esrgan_config.py:73-74)
    ((4, 3, 512, 512), 1 / 4, True),
    ((2, 3, 384, 256), 1 / 2, True),
    ((2, 3, 384, 256), 1 / 8, True),
    ((2, 3, 64, 48), 4, True),
    ((1, 3, 301, 203), 0.9, True),
    ((3, 64, 64), 1 / 4, False),             # no padding at the end of either side: the reference raises, the result is defined
    ((3, 64, 64), 1 / 8, True),
    ((2, 3, 40, 56), 8, True),
])
def test_training_shapes_vs_oracle(shape, scale, aa):
    rng = np.random.RandomState(sum(shape) + int(scale * 1000))
    x = u8_grid(rng, *shape)
    got = resize(x, scale, aa)
    check_vs_oracle(f"{shape} x {scale:.4g}{'' if aa else ' (no antialiasing)'}", x, got, scale, aa)


def test_batch_rows_and_repeats_are_bitwise_stable():
    rng = np.random.RandomState(5)
    x = torch.from_numpy(u8_grid(rng, 6, 3, 128, 128)).to(DEV)
    y = resize(x, 1 / 4)
    assert torch.equal(resize(x, 1 / 4), y)                        # two calls, identical bits
    for i in range(x.shape[0]):
        assert torch.equal(resize(x[i], 1 / 4), y[i]), i           # image i of the batch == the same image alone
        assert torch.equal(resize(x[i:i + 1], 1 / 4)[0], y[i]), i
    up = resize(x[:2], 2)
    assert torch.equal(resize(x[1], 2), up[1]) and torch.equal(resize(x[:2], 2), up)


def test_consistent_with_the_half_size_planes_of_niqe(golden_dir):
    """what is already pinned: NIQE's half-size planes, recorded from the reference's own 0.5x resize (tests/golden/niqe.npz), fed as
    tests/test_niqe_gpu.py feeds srganfd_resize_half"""
    _, _, _, ncases = NO.load_cases(os.path.join(golden_dir, "niqe.npz"))
    for name, c in ncases.items():
        luma = torch.from_numpy(c["luma"]).to(DEV)                 # (N, h, w) fp64 integers
        got = resize((luma / 255).float(), 0.5)
        h, w = luma.shape[-2:]
        b, widen, delta = bounds(h, w, 0.5, True)
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - c["half"]).max())
        print(f"niqe case {name}: vs recorded half-size plane {err:.3e} = {err / b:.3f} B (table delta {delta:.1e})")
        assert tuple(got.shape) == c["half"].shape
        assert delta <= DELTA_MAX
        assert err <= 2 * b + widen


def u8_batches(rng, count, n, h, w, with_lr=False):
    out = []
    for _ in range(count):
        b = {"gt": torch.from_numpy(rng.randint(0, 256, size=(n, h, w, 3)).astype(np.uint8))}
        if with_lr:
            b["lr"] = torch.from_numpy(rng.rand(n, 3, h // 4, w // 4).astype(np.float32))
        out.append(b)
    return out


def test_prefetcher_synthesizes_lr():
    from sr_gan_fd_amd.dataset import CUDAPrefetcher
    from sr_gan_fd_amd.imgproc import image_resize, image_to_tensor_u8
    rng = np.random.RandomState(11)
    n, h, w = 4, 96, 128
    loader = u8_batches(rng, 3, n, h, w)
    pf = CUDAPrefetcher(loader, DEV, ingest_u8=True, synthesize_lr=4)
    assert len(pf) == 3
    for i in range(3):
        batch = pf.next()
        assert batch is not None and set(batch) == {"gt", "lr"}
        gt, lr = batch["gt"], batch["lr"]
        assert gt.shape == (n, 3, h, w) and gt.dtype == torch.float32
        assert lr.shape == (n, 3, h // 4, w // 4) and lr.dtype == torch.float32 and lr.is_cuda
        assert torch.equal(gt, image_to_tensor_u8(loader[i]["gt"].to(DEV)))
        want = image_resize(gt, 0.25)                              # afterwards, on the consumer stream
        torch.cuda.synchronize()
        assert torch.equal(lr, want), i
    assert pf.next() is None
    pf.reset()
    assert torch.equal(pf.next()["lr"], image_resize(image_to_tensor_u8(loader[0]["gt"].to(DEV)), 0.25))


def test_prefetcher_keeps_a_given_lr_and_defaults_to_none():
    from sr_gan_fd_amd.dataset import CUDAPrefetcher
    rng = np.random.RandomState(12)
    loader = u8_batches(rng, 2, 2, 64, 64, with_lr=True)
    pf = CUDAPrefetcher(loader, DEV, ingest_u8=True, synthesize_lr=4)
    for i in range(2):
        batch = pf.next()
        assert torch.equal(batch["lr"].cpu(), loader[i]["lr"])
    plain = CUDAPrefetcher(u8_batches(rng, 2, 2, 64, 64), DEV, ingest_u8=True)
    batch = plain.next()
    assert set(batch) == {"gt"} and plain.synthesize_lr is None
    with pytest.raises(ValueError):
        CUDAPrefetcher(loader, DEV, synthesize_lr=0)
