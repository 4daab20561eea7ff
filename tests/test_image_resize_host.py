"""CPU-only tests of imgproc.image_resize's host side and of trainer.StepLR.

Tables: the package's float32 table builder (sr_gan_fd_amd/imgproc.py:_resize_tables_host) and the oracle's (tests/resize_oracle.py)
against the tables the reference built for every case of tests/golden/image_resize.npz: first indices equal and weights BIT-IDENTICAL
(a float32 restatement in the reference's order of operations; the fixture was recorded with the same torch CPU kernels).
Oracle: fp64 accumulation on float32 tables against every recorded float32 output, within the derived bound B of
tests/resize_oracle.py.  Measured here: the reference lies within 0.086 B of the oracle over the 15 cases (largest at x2).
Binding: srganfd_imresize is declared, bound and exported, the ABI version is still 7, and the entry point validates its arguments in
dry-run mode, where nothing is launched."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import resize_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_NAMES = RO.CASE_NAMES


@pytest.fixture(scope="module")
def cases(golden_dir):
    return RO.load_cases(os.path.join(golden_dir, "image_resize.npz"))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def sides(c):
    """(side name, in length, out length, recorded weights, recorded first samples, recorded (sym_len_s, sym_len_e)) of one case"""
    h, w = c["input"].shape[-2:]
    return (("h", h, math.ceil(h * c["scale"]), c["weights_h"], c["first_h"], tuple(c["sym"][:2])),
            ("w", w, math.ceil(w * c["scale"]), c["weights_w"], c["first_w"], tuple(c["sym"][2:])))


def test_fixture_holds_every_case(cases):
    assert list(cases) == CASE_NAMES
    for name, c in cases.items():
        h, w = c["input"].shape[-2:]
        assert c["output"].dtype == np.float32
        assert c["output"].shape == c["input"].shape[:-2] + (math.ceil(h * c["scale"]), math.ceil(w * c["scale"])), name
    assert cases["x15_77x64_2d"]["input"].ndim == 2 and cases["s09_301x203"]["input"].shape[0] == 1
    assert cases["q65x66_plain"]["sym"][0] == 0            # a side without padding at its start, which the reference still runs


@pytest.mark.parametrize("name", CASE_NAMES)
def test_package_tables_are_the_references(cases, name):
    from sr_gan_fd_amd.imgproc import _resize_tables_host
    c = cases[name]
    for side, n, out, want_w, want_first, want_sym in sides(c):
        w, first, pad_s, pad_e = _resize_tables_host(n, out, c["scale"], c["antialiasing"])
        w, first = w.numpy(), first.numpy()
        assert w.dtype == np.float32 and first.dtype == np.int32
        assert w.shape == want_w.shape and (first == want_first).all(), (name, side)
        assert (bits(w) == bits(want_w)).all(), (name, side, float(np.abs(w - want_w).max()))
        assert (pad_s, pad_e) == want_sym, (name, side)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_oracle_tables_are_the_references(cases, name):
    """the oracle keeps every column; the reference dropped the outermost pair, which holds zeros"""
    c = cases[name]
    for side, n, out, want_w, want_first, _ in sides(c):
        w, first = RO.tables(n, out, c["scale"], c["antialiasing"])
        assert w.dtype == np.float32 and w.shape == (out, want_w.shape[1] + 2), (name, side)
        assert (first + 1 == want_first).all(), (name, side)
        assert (bits(w[:, 1:-1]) == bits(want_w)).all(), (name, side)
        assert (w[:, 0] == 0).all() and (w[:, -1] == 0).all(), (name, side)
        assert RO.table_delta(w, first, want_w, want_first) == 0.0


@pytest.mark.parametrize("name", CASE_NAMES)
def test_oracle_reproduces_reference(cases, name):
    c = cases[name]
    h, w = c["input"].shape[-2:]
    b = RO.bound_for(h, w, c["scale"], c["antialiasing"])
    got = RO.resize(c["input"], c["scale"], c["antialiasing"])
    err = float(np.abs(got - c["output"].astype(np.float64)).max())
    print(f"case {name}: B {b:.3e}, reference vs oracle {err:.3e} = {err / b:.3f} B")
    assert got.shape == c["output"].shape
    assert err <= b


def test_bound_values():
    """B as the issue states it: 3.4e-6 at 1/4, 6.0e-6 at 1/8, 1.6e-6 when enlarging (P = 18, 34, 6 taps)"""
    for (n, scale), want in (((128, 1 / 4), 3.4e-6), ((128, 1 / 8), 6.0e-6), ((32, 4), 1.6e-6)):
        b = RO.bound_for(n, n, scale)
        assert abs(b / want - 1) < 0.05, (scale, b)


def test_errors_need_no_gpu():
    from sr_gan_fd_amd import _abi as A
    from sr_gan_fd_amd.imgproc import image_resize
    with pytest.raises(A.SrganfdError, match="on the GPU"):
        image_resize(torch.rand(3, 64, 64), 1 / 4)
    with pytest.raises(A.SrganfdError):
        image_resize(np.zeros((64, 64, 3), dtype=np.float32), 1 / 4)
    with pytest.raises(ValueError, match="scale_factor"):
        image_resize(torch.rand(3, 64, 64), 0)
    with pytest.raises(ValueError, match="scale_factor"):
        image_resize(torch.rand(3, 64, 64), -0.5)
    with pytest.raises(ValueError, match="height"):
        image_resize(torch.rand(3, 4, 4), 1 / 4)               # padding longer than the image: the reference dies in copy_
    with pytest.raises(ValueError, match="width"):
        image_resize(torch.rand(3, 64, 4), 1 / 4)


def test_symbol_declared_bound_exported():
    from sr_gan_fd_amd import _abi as A
    hdr = open(os.path.join(ROOT, "include", "srganfd.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", A.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert "srganfd_imresize" in A.SYMBOLS
    assert re.search(r"\bsrganfd_imresize\s*\(", hdr)
    assert "srganfd_imresize" in exported
    assert int(re.search(r"^#define\s+SRGANFD_ABI_VERSION\s+(\d+)", hdr, re.M).group(1)) == 7
    assert A.ABI_VERSION == 7 and A.lib().srganfd_abi_version() == 7


def test_argument_validation_dry_run():
    from sr_gan_fd_amd import _abi as A
    L = A.lib()
    A.set_dry_run(True)
    try:
        p = 4096                                            # a non-null address; nothing is dereferenced in dry-run mode

        def call(planes=96, h=512, w=512, oh=128, ow=128, th=16, tw=16, src=p, wt=p, first=p, dst=p):
            return L.srganfd_imresize(src, planes, h, w, oh, ow, wt, first, th, wt, first, tw, dst, 0)

        def err():
            return L.srganfd_last_error().decode()

        assert call() == 0
        for s in (1 / 8, 1 / 4, 1 / 3, 1 / 2, 0.7, 1, 2, 3, 4, 8):          # every scale of [1/8, 8] finds a tile, either antialiasing
            for taps in (4, math.ceil(4 / min(s, 1))):
                for n in (7, 64, 301, 2048):
                    if math.ceil(n * s) >= 1:
                        assert call(3, n, n, math.ceil(n * s), math.ceil(n * s), taps, taps) == 0, (s, taps, n, err())
        assert call(src=None) == -1 and "null" in err()
        assert call(dst=None) == -1 and call(wt=None) == -1 and call(first=None) == -1
        for kw in ({"planes": 0}, {"h": 0}, {"w": -1}, {"oh": 0}, {"ow": 0}, {"th": 0}, {"tw": 0}):
            assert call(**kw) == -1 and "positive" in err(), kw
        assert call(planes=65536) == -1 and "planes" in err()
        assert call(h=4096, w=4096, oh=16, ow=16, th=1024, tw=1024) == -1 and "LDS" in err()    # 1/256: no tile holds one output's footprint
    finally:
        A.set_dry_run(False)


@pytest.mark.parametrize("step_size,gamma", [(3, 0.5), (5, 0.5), (3, 0.1), (5, 0.1)])
def test_step_lr_mirror_follows_torch_and_exchanges_state(step_size, gamma):
    """trainer.StepLR == torch.optim.lr_scheduler.StepLR (ESRGAN/rrdbnet_config.py:77-78, one step per epoch: train_rrdbnet.py:205-210)
    on the fused optimizer: the same rate at every epoch, exactly (both multiply the current rate by gamma in double precision), and
    the two load each other's state_dict in the middle of a run."""
    from sr_gan_fd_amd.trainer import FlatAdamEMA, StepLR
    fused = FlatAdamEMA(torch.zeros(1), 2e-4, (0.9, 0.99), 1e-4)
    ref_opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], 2e-4)
    mine, ref = StepLR(fused, step_size, gamma), torch.optim.lr_scheduler.StepLR(ref_opt, step_size, gamma)
    assert set(ref.state_dict()) - {"_is_initial"} <= set(mine.state_dict())
    for key in ("step_size", "gamma", "base_lrs", "last_epoch", "_step_count", "_last_lr"):
        assert mine.state_dict()[key] == ref.state_dict()[key], key
    mine2 = ref2 = ref_opt2 = fused2 = None
    for epoch in range(13):
        assert mine.get_last_lr() == ref.get_last_lr() and fused.lr == ref_opt.param_groups[0]["lr"], epoch
        assert mine.last_epoch == ref.last_epoch == epoch
        if mine2 is not None:
            assert mine2.get_last_lr() == ref2.get_last_lr() == mine.get_last_lr() and fused2.lr == fused.lr, epoch
        if epoch == 4:
            # resume in the middle: each implementation continues from the other's state
            fused2 = FlatAdamEMA(torch.zeros(1), 1.0, (0.9, 0.99), 1e-4)
            mine2 = StepLR(fused2, 1, 0.9)
            mine2.load_state_dict(ref.state_dict())
            ref_opt2 = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], 1.0)
            ref2 = torch.optim.lr_scheduler.StepLR(ref_opt2, 1, 0.9)
            ref2.load_state_dict(mine.state_dict())
            ref_opt2.param_groups[0]["lr"] = ref2.get_last_lr()[0]      # torch restores the rate with the optimizer's own state
            assert fused2.lr == fused.lr and mine2.last_epoch == ref.last_epoch and mine2.step_size == step_size
        ref_opt.step()
        mine.step()
        ref.step()
        if mine2 is not None:
            ref_opt2.step()
            mine2.step()
            ref2.step()
    assert abs(fused.lr / (2e-4 * gamma ** (13 // step_size)) - 1) < 1e-12          # last_epoch is 13 now
    with pytest.raises(ValueError):
        StepLR(fused, 0)
