"""CPU-only LPIPS tests: constructor spellings and refusals, host-side shape checks, state-dict handling, the workspace query
against the map sizes the torch-CPU restatement (tests/lpips_oracle.py) produces, the new C entry points (declared, bound,
exported, validating in dry-run mode where nothing is launched), and the oracle's own fp32-versus-fp64 gap G, which sets the
scale of the GPU tolerances (tests/test_lpips_gpu.py).

G measured on an x86-64 host (largest relative gap over the five per-layer values and the total; normalize False / True;
torch's CPU kernels choose their summation order by machine, so another host prints other figures of this size):
  case A 1x3x31x31    1.40e-06 / 7.77e-07
  case B 2x3x67x90    1.27e-06 / 2.23e-07
  case C 3x3x128x160  7.04e-07 / 2.43e-07"""
import ctypes as C
import os
import re
import subprocess
import warnings

import pytest
import torch

from tests import lpips_oracle as LO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("srganfd_lpips_conv", "srganfd_lpips_head", "srganfd_lpips_workspace_bytes")


def quiet(**kw):
    from sr_gan_fd_amd.image_quality_assessment import LPIPS
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return LPIPS(**kw)


def test_script_spellings_construct():
    """train_bsrgan.py:115 writes LPIPS(net='alex'), train_aesrgan.py:133 LPIPS(net=cfg.lpips_net); .to / .eval / .cuda exist"""
    from sr_gan_fd_amd.image_quality_assessment import LPIPS
    from sr_gan_fd_amd import lpips as mod
    mod._warned = False
    with pytest.warns(UserWarning, match="NOT the published"):
        m = LPIPS(net="alex")
    lpips_net = "alex"
    m2 = quiet(net=lpips_net)
    assert isinstance(m, torch.nn.Module) and not m.training and hasattr(m, "cuda")
    assert m.to(torch.device("cpu")) is m and m.eval() is m
    assert all(not p.requires_grad for p in m.parameters())
    # seeded: two constructions hold the same values; convs He-scaled with zero bias, lin weights non-negative
    for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    assert m.state_dict()["net.slice2.3.bias"].abs().max() == 0 and all(m.state_dict()[f"lin{k}.model.1.weight"].min() >= 0 for k in range(5))


@pytest.mark.parametrize("kw,word", [({"net": "vgg"}, "net='alex'"), ({"net": "squeeze"}, "net='alex'"), ({"version": "0.0"}, "version='0.1'"),
                                     ({"spatial": True}, "spatial=False"), ({"lpips": False}, "lpips=True")])
def test_unsupported_options_raise(kw, word):
    from sr_gan_fd_amd._abi import SrganfdError
    from sr_gan_fd_amd.image_quality_assessment import LPIPS
    with pytest.raises(SrganfdError) as e:
        LPIPS(**kw)
    assert word in str(e.value)


def test_shape_checks_on_the_host():
    """every refusal comes before any launch: these are CPU tensors, and a shape that passes the checks is refused only for
    not being on the GPU"""
    from sr_gan_fd_amd._abi import SrganfdError
    m = quiet()
    with pytest.raises(SrganfdError, match="at least 31"):
        m(torch.rand(1, 3, 30, 40), torch.rand(1, 3, 30, 40))
    with pytest.raises(SrganfdError, match="at least 31"):
        m(torch.rand(1, 3, 40, 30), torch.rand(1, 3, 40, 30))
    with pytest.raises(SrganfdError, match="on the GPU"):
        m(torch.rand(1, 3, 31, 31), torch.rand(1, 3, 31, 31))
    with pytest.raises(SrganfdError, match="3-channel"):
        m(torch.rand(1, 1, 64, 64), torch.rand(1, 1, 64, 64))
    with pytest.raises(SrganfdError, match="differ in shape"):
        m(torch.rand(1, 3, 64, 64), torch.rand(1, 3, 64, 65))
    with pytest.raises(SrganfdError, match="N,3,H,W"):
        m(torch.rand(3, 64, 64), torch.rand(3, 64, 64))


def test_smallest_input_derivation():
    """31 is the smallest size torch's own ops accept for this trunk, 30 fails at the second pool"""
    sd = LO.synthetic_state_dict()
    t = LO.taps(torch.rand(1, 3, 31, 31), sd, torch.float32)
    assert [tuple(x.shape[2:]) for x in t] == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]
    with pytest.raises(RuntimeError):
        LO.taps(torch.rand(1, 3, 30, 31), sd, torch.float32)


def test_state_dict_round_trip_and_forms(tmp_path):
    sd = LO.synthetic_state_dict()
    m = quiet()
    assert set(m.state_dict().keys()) == set(sd.keys())
    m.load_state_dict(sd)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # round trip through a second module
    m2 = quiet()
    m2.load_state_dict(m.state_dict())
    assert all(torch.equal(v, sd[k]) for k, v in m2.state_dict().items())
    # a state dict saved where the package is installed also carries the ModuleList names; duplicates are ignored
    with_alias = dict(sd)
    for k in range(5):
        with_alias[f"lins.{k}.model.1.weight"] = sd[f"lin{k}.model.1.weight"].clone()
    m3 = quiet()
    m3.load_state_dict(with_alias)
    assert all(torch.equal(v, sd[k]) for k, v in m3.state_dict().items())
    # the alias alone names the layer
    only_alias = {k: v for k, v in with_alias.items() if not re.match(r"lin\d\.", k)}
    m4 = quiet()
    m4.load_state_dict(only_alias)
    assert all(torch.equal(v, sd[k]) for k, v in m4.state_dict().items())
    # an alias that disagrees with its layer is an error, not a silent choice
    from sr_gan_fd_amd._abi import SrganfdError
    with_alias["lins.2.model.1.weight"] = with_alias["lins.2.model.1.weight"] + 1
    with pytest.raises(SrganfdError, match="lins.2"):
        quiet().load_state_dict(with_alias)
    # the two-file form: torchvision alexnet state dict (plain and wrapped) + the package's lin file
    backbone, lins = LO.two_file_form(sd)
    torch.save(backbone, str(tmp_path / "alexnet.pth"))
    torch.save({"state_dict": backbone}, str(tmp_path / "alexnet_wrapped.pth"))
    torch.save(lins, str(tmp_path / "alex.pth"))
    for name in ("alexnet.pth", "alexnet_wrapped.pth"):
        m5 = quiet(model_path=str(tmp_path / "alex.pth"), backbone_weights_path=str(tmp_path / name))
        assert all(torch.equal(v, sd[k]) for k, v in m5.state_dict().items())
    with pytest.raises(SrganfdError, match="nowhere.pth"):
        quiet(model_path=str(tmp_path / "nowhere.pth"))
    torch.save({k: v for k, v in backbone.items() if k != "features.6.bias"}, str(tmp_path / "partial.pth"))
    with pytest.raises(SrganfdError, match="features.6.bias"):
        quiet(backbone_weights_path=str(tmp_path / "partial.pth"))


def test_workspace_query_matches_oracle_maps():
    from sr_gan_fd_amd import _abi as A
    from sr_gan_fd_amd import lpips as mod
    L = A.lib()
    sd = LO.synthetic_state_dict()
    for n, h, w in ((2, 67, 90), (1, 31, 31), (3, 128, 160)):
        shapes = [tuple(t.shape[2:]) for t in LO.taps(torch.rand(1, 3, h, w), sd, torch.float32)]
        if (h, w) == (67, 90):
            assert shapes == [(16, 21), (7, 10), (3, 4), (3, 4), (3, 4)]
            pool1 = tuple(torch.nn.functional.max_pool2d(torch.zeros(1, 1, 16, 21), 3, 2).shape[2:])
            pool2 = tuple(torch.nn.functional.max_pool2d(torch.zeros(1, 1, 7, 10), 3, 2).shape[2:])
            assert (pool1, pool2) == ((7, 10), (3, 4))
        assert [tuple(s) for s in mod.map_sizes(h, w)] == shapes
        floats = sum(hk * wk * (2 * n * c + n) for (hk, wk), c in zip(shapes, LO.CHANNELS))
        assert L.srganfd_lpips_workspace_bytes(n, h, w) == 4 * floats
    assert L.srganfd_lpips_workspace_bytes(1, 30, 31) == -1 and "at least 31" in L.srganfd_last_error().decode()
    assert L.srganfd_lpips_workspace_bytes(1, 31, 30) == -1
    assert L.srganfd_lpips_workspace_bytes(0, 64, 64) == -1


def test_new_symbols_declared_bound_exported():
    from sr_gan_fd_amd import _abi as A
    hdr = open(os.path.join(ROOT, "include", "srganfd.h")).read()
    import glob
    srcs = "\n".join(open(f).read() for f in sorted(glob.glob(os.path.join(ROOT, "sr_gan_fd_amd", "csrc", "*.hip"))))
    nm = subprocess.run(["nm", "-D", "--defined-only", A.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in NEW_SYMBOLS:
        assert name in A.SYMBOLS, f"{name} missing from _abi.SYMBOLS"
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} not declared in include/srganfd.h"
        # a definition (a type, the name, an argument list, a body), not a call: entry points live beside the kernels they launch
        assert re.search(r'^(extern "C" )?[\w \*]+\b%s\s*\([^;{]*\{' % name, srcs, re.M), f"{name} not defined in any csrc/*.hip"
        assert name in exported, f"{name} not exported by {A.LIB_PATH}"
    assert A.lib().srganfd_abi_version() == 7 and A.ABI_VERSION == 7
    # the binding's structures have the header's sizes (x86-64: 14 int32, 3 + 3 pointers, 8 int64, 6 floats, 2 pad words)
    assert C.sizeof(A.LpipsConvArgs) == 14 * 4 + 6 * 8 + 8 * 8 + 6 * 4 + 2 * 4
    assert C.sizeof(A.LpipsTap) == 2 * 8 + 4 * 4


def conv_args(A, **kw):
    a = A.LpipsConvArgs()
    p = 4096                                            # a non-null, aligned address; nothing is dereferenced in dry-run mode
    base = dict(n=4, h_in=67, w_in=90, cin=3, cout=64, ksize=11, stride=4, pad=2, pool=0, first=1, normalize=0, h_out=16, w_out=21,
                x=None, in0=p, in1=p, w=p, bias=p, y=p)
    base.update(kw)
    for k, v in base.items():
        setattr(a, k, v)
    a.scale = (C.c_float * 3)(*LO.SCALE)
    return a


def test_argument_validation_dry_run():
    from sr_gan_fd_amd import _abi as A
    L = A.lib()
    A.set_dry_run(True)
    try:
        p = 4096

        def err():
            return L.srganfd_last_error().decode()

        def conv(**kw):
            return L.srganfd_lpips_conv(C.byref(conv_args(A, **kw)), 0)

        second = dict(first=0, in0=None, in1=None, x=p, cin=64, cout=192, ksize=5, stride=1, pad=2, pool=1, h_in=16, w_in=21, h_out=7, w_out=10)
        third = dict(second, cin=192, cout=384, ksize=3, pad=1, h_in=7, w_in=10, h_out=3, w_out=4)
        fourth = dict(third, cin=384, cout=256, pool=0, h_in=3, w_in=4)
        for good in ({}, second, third, fourth, dict(fourth, h_in=1, w_in=1, h_out=1, w_out=1)):
            assert conv(**good) == 0, (good, err())
        for bad, word in ((dict(h_out=17), "does not follow"), (dict(cout=96), "multiple of 64"), (dict(cin=4), "no kernel"),
                          (dict(n=3), "even batch"), (dict(in1=None), "both images"), (dict(w=None), "null"),
                          (dict(second, cin=48), "multiple of 32"), (dict(second, ksize=7), "no kernel"),
                          (dict(second, x=None), "input map"), (dict(second, x=p + 4), "unaligned"),
                          (dict(third, h_in=2, h_out=1), "smaller than the 3 x 3 pool"), (dict(second, first=1), "no kernel")):
            assert conv(**bad) == -1 and word in err(), (bad, err())
        assert L.srganfd_lpips_conv(None, 0) == -1

        def head(ntaps=1, n=2, h=7, w=10, c=384, maps=p, lin=p, out=p, ws=p):
            t = (A.LpipsTap * 5)()
            for i in range(5):
                t[i].maps, t[i].lin, t[i].h, t[i].w, t[i].c = maps, lin, h, w, c
            return L.srganfd_lpips_head(t, ntaps, n, out, ws, 0)

        assert head() == 0 and head(ntaps=5, c=64, h=1, w=1) == 0
        for bad, word in ((dict(c=96), "multiple of 64"), (dict(c=448), "multiple of 64"), (dict(ntaps=6), "taps"), (dict(ntaps=0), "taps"),
                          (dict(n=0), "n 0"), (dict(h=0), "0 x 10"), (dict(maps=None), "null"), (dict(out=None), "null")):
            assert head(**bad) == -1 and word in err(), (bad, err())
    finally:
        A.set_dry_run(False)


def test_oracle_reference_gap():
    """G: how far torch's own fp32 arithmetic (the reference's) lies from the fp64 values on the GPU tests' cases.  The GPU tests
    allow 8 G.  fp32 has a 6e-8 unit roundoff and the sums have up to 3456 terms, so G must stay far below 1e-3; were it not,
    the cases would be ill-conditioned and say nothing."""
    for name in LO.CASES:
        for normalize in (False, True):
            c = LO.case(name, normalize)
            print(f"case {name} normalize={normalize}: total {c['want'][0].tolist()}  G {c['G']:.3e}  per value "
                  + " ".join(f"{g:.2e}" for g in c["gaps"]))
            assert 0 < c["G"] < 1e-4
            assert all(v.min().item() > 1e-6 for v in [c["want"][0]] + c["want"][1])       # no value at zero: a relative bound has meaning
            # ReLU zeroes a real share of every tap (biases of both signs), and leaves a real share
            for t in c["want"][2]:
                share = (t == 0).double().mean().item()
                assert 0.05 < share < 0.95, share
