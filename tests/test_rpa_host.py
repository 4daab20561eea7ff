"""Host-side checks of RPA, US and Generator_RPA (no GPU: the library runs in dry-run mode, where every entry point validates its
arguments and launches nothing): the float64 oracle (tests/rpa_oracle.py) against the reference's own outputs (tests/golden/rpa.npz,
written by tests/golden/make_golden_rpa.py), the three classes' keys, shapes and seeded initial values, copies, the conditions the
GPU tests' cases were chosen under, every SRGANFD_EINVAL path of srganfd_pixel_gate, and the sequence of calls a forward + backward
of each module makes.

Conditions on the cases (rpa_oracle.CASES; the seeds are the first that meet all of them, found by a search on the CPU):
  quantiles    the 5 % and 95 % quantiles of sigmoid(a) over a case lie below 0.2 and above 0.8: the gate is not the near-constant 1.5
               of the reference's initialisation, under which a wrong gate would hide below the tolerance.
  zero margin  in the float64 run no LeakyReLU pre-activation lies within 2e-6 of its tensor's largest magnitude of zero (about 16
               float32 epsilons; the float32 run's own deviation is 0.5-1.2e-6): a pre-activation cannot take the other branch
               under another summation order (the effect tests/test_aesrgan_gpu.py describes).
  E caps       the relative L2 gap E of the oracle with a 16-bit type's rounding points to the plain float64 oracle is at most 0.05
               for float16 and 0.15 for bfloat16, per tensor: the GPU tests' bounds max(2 E, 8 G) stay far below a whole-tensor mistake.
"""
import copy
import os
import pickle

import numpy as np
import pytest
import torch

from tests import rpa_oracle as RO
from tests.util import checksum

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rpa.npz")
EINVAL = -1


@pytest.fixture(scope="module")
def golden():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture
def dry_run():
    from sr_gan_fd_amd import _abi as A
    A.set_dry_run(True)
    yield A
    A.set_dry_run(False)


def test_fixture_is_small(golden):
    assert os.path.getsize(FIXTURE) < 200 << 10
    for k, v in golden.items():
        if k.startswith("init."):
            continue
        f64 = k.endswith((".out", ".dx", ".sigmoid_q")) or ".grad." in k
        assert v.dtype == (np.float64 if f64 else np.float16), k


@pytest.mark.parametrize("low_res", [True, False], ids=["low_res", "reference_order"])
@pytest.mark.parametrize("name", list(RO.FIXTURE_CASES))
def test_oracle_reproduces_the_reference(golden, name, low_res):
    kind, scale, x, state, d_out = RO.case_inputs(name)
    assert np.array_equal(golden[name + ".x"].astype(np.float32), x.numpy())                       # the recipe still gives the fixture's inputs
    assert np.array_equal(golden[name + ".d_out"].astype(np.float32), d_out.numpy())
    for k, v in state.items():
        assert np.array_equal(golden[name + ".state." + k].astype(np.float32), v.numpy()), k
    kw = {} if kind == "rpa" else {"low_res": low_res}
    res = RO.run_case(kind, x, state, scale, d_out=d_out, **kw)
    want = {"out": golden[name + ".out"], "dx": golden[name + ".dx"], **{k: golden[name + ".grad." + k] for k in state}}
    assert set(want) == set(res)
    for k, w in want.items():
        w = torch.from_numpy(w)
        assert res[k].shape == w.shape, k
        assert RO.max_gap(res[k], w) <= 1e-12, k


@pytest.mark.parametrize("cls", ["RPA", "US", "Generator_RPA"])
def test_classes_have_the_references_keys_shapes_and_initial_values(golden, cls):
    from sr_gan_fd_amd import model as M
    make = {"RPA": lambda: M.RPA(64), "US": lambda: M.US(64, 2), "Generator_RPA": lambda: M.Generator_RPA(scale=2, num_block=2)}[cls]
    torch.manual_seed(0)
    m = make()
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in golden[f"init.{cls}.keys"]]
    for v, shape, want in zip(sd.values(), golden[f"init.{cls}.shapes"], golden[f"init.{cls}.checksums"]):
        assert list(v.shape) == [int(s) for s in shape[:v.dim()]]
        assert np.allclose(checksum(v), want, rtol=1e-9, atol=1e-9)
    assert m.compute_dtype is None and cls in M.__all__
    kind = {"RPA": "rpa", "US": "us", "Generator_RPA": "gen"}[cls]
    assert list(sd) == [n + s for n, _, _, _ in RO.conv_shapes(kind, 64, 2, 2) for s in (".weight", ".bias")]


def test_generator_attributes_and_factory(capsys):
    from sr_gan_fd_amd import model as M
    for scale, n_us in ((1, 0), (2, 1), (3, 2), (4, 2), (8, 3)):
        g = M.Generator_RPA(scale=scale, num_block=1)
        assert g.scale == scale and len(g.us) == n_us and all(u.scale == 2 for u in g.us)
    capsys.readouterr()
    g = M.__dict__["gen_rpa2x"]()
    assert capsys.readouterr().out == "* Generator_RPA 2x\n"
    assert isinstance(g, M.Generator_RPA) and len(g.rpa) == 20 and len(g.us) == 1 and g.scale == 2 and "gen_rpa2x" in M.__all__


def test_deepcopy_and_pickle_give_independent_modules(dry_run):
    from sr_gan_fd_amd import model as M
    from sr_gan_fd_amd.engine_rpa import rpa_engine
    torch.manual_seed(1)
    m = M.Generator_RPA(scale=2, num_block=1)
    x = torch.rand(1, 3, 4, 5)
    m(x)
    for other in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert list(other.state_dict()) == list(m.state_dict())
        assert all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), m.state_dict().values()))
        assert other(x).shape == (1, 3, 8, 10)
        e0, e1 = rpa_engine(m, "gen"), rpa_engine(other, "gen")
        assert e0 is not e1 and e0.fp.flat.data_ptr() != e1.fp.flat.data_ptr()
        with torch.no_grad():
            other.conv1.weight.add_(1.0)
        assert not torch.equal(other.conv1.weight, m.conv1.weight)


@pytest.mark.parametrize("name", list(RO.CASES) + list(RO.FIXTURE_CASES))
def test_gate_is_not_degenerate(name, golden):
    lo, hi = RO.sigmoid_quantiles(RO.runs(name)["probe"])
    assert lo < 0.2 and hi > 0.8, (lo, hi)
    if name in RO.FIXTURE_CASES:
        # ... and so did the reference itself.  The same numbers for an RPA; a US evaluates its sigmoid at the high resolution
        # there, every value four times, which weighs the quantiles of a case with US blocks differently
        rlo, rhi = golden[name + ".sigmoid_q"]
        assert rlo < 0.2 and rhi > 0.8
        if RO.FIXTURE_CASES[name][0] == "rpa":
            assert np.allclose([rlo, rhi], [lo, hi], rtol=1e-9)


@pytest.mark.parametrize("name", list(RO.CASES))
def test_no_pre_activation_near_zero(name):
    assert RO.zero_margin(RO.runs(name)["probe"]) > 2e-6


@pytest.mark.parametrize("name", list(RO.CASES))
def test_oracle_alone_meets_the_caps(name):
    r = RO.runs(name)
    for k, ref in r["f64"].items():
        e16, ebf = RO.l2_gap(r["f16"][k], ref), RO.l2_gap(r["bf16"][k], ref)
        print("%-10s %-28s E f16 %.2e  bf16 %.2e  G(max) %.2e" % (name, k, e16, ebf, RO.max_gap(r["f32"][k], ref)))
        assert e16 <= 0.05 and ebf <= 0.15, (k, e16, ebf)


def test_abi_version_stays_7():
    from sr_gan_fd_amd import _abi as A
    assert A.lib().srganfd_abi_version() == A.ABI_VERSION == 7
    assert "srganfd_pixel_gate" in A.SYMBOLS and hasattr(A.lib(), "srganfd_pixel_gate")


def test_pixel_gate_refuses_bad_arguments(dry_run):
    from sr_gan_fd_amd import ops
    A = dry_run
    L = A.lib()
    npix, c = 35, 64
    t = {k: torch.zeros(npix, 96) for k in ("x", "a", "z", "dx", "da")}
    V = lambda k, **kw: A.view(t[k], **{"c0": 32, **kw})

    def call(args):
        return L.srganfd_pixel_gate(*args, None), L.srganfd_last_error().decode()

    def fwd(dtype=A.F32, npix=npix, c=c, **v):
        vs = {k: V(k) for k in ("x", "a", "z")}
        vs.update(v)
        return ops.pixel_gate_args(dtype, npix, c, vs["x"], vs["a"], z=vs["z"])

    def bwd(dtype=A.F16, npix=npix, c=c, **v):
        vs = {"x": V("x"), "a": V("a"), "dz": V("z"), "dx": V("dx"), "da": V("da")}
        vs.update(v)
        return ops.pixel_gate_args(dtype, npix, c, vs["x"], vs["a"], dz=vs["dz"], dx=vs["dx"], da=vs["da"])
    assert call(fwd())[0] == 0 and call(bwd())[0] == 0
    assert call(bwd(da=V("z")))[0] == 0                                      # da over dz, in place
    assert call(fwd(c=32, z=A.view(t["x"], c0=64)))[0] == 0                  # disjoint slices of one buffer
    for make, names in ((fwd, ("x", "a", "z")), (bwd, ("x", "a", "dz", "dx", "da"))):
        what = "pixel_gate(bwd)" if make is bwd else "pixel_gate:"
        for n in names:
            rc, msg = call(make(**{n: A.NULL_VIEW}))
            if make is bwd and n == "dz":                                     # (without dz the arguments ARE a forward call's: z is what is missing)
                assert rc == EINVAL and "null pointer (z)" in msg, msg
                continue
            assert rc == EINVAL and "null pointer (%s)" % n in msg and what in msg, (n, msg)
            key = "z" if n == "dz" else n
            rc, msg = call(make(**{n: A.view(t[key], c0=32, planar=1)}))
            assert rc == EINVAL and "planar" in msg and what in msg, (n, msg)
            rc, msg = call(make(**{n: A.view(t[key], c0=4)}))
            assert rc == EINVAL and "misaligned" in msg, (n, msg)
            rc, msg = call(make(**{n: A.view(t[key], cstride=100, c0=32)}))
            assert rc == EINVAL and "misaligned" in msg, (n, msg)
            rc, msg = call(make(**{n: A.view(t[key].view(-1)[1:], cstride=96, c0=32)}))      # 4 bytes off a 16-byte boundary
            assert rc == EINVAL and "misaligned" in msg, (n, msg)
            rc, msg = call(make(**{n: A.view(t[key], c0=64)}))
            assert rc == EINVAL and "exceeds" in msg, (n, msg)
        for bad_c in (0, -32, 16, 48):
            rc, msg = call(make(c=bad_c))
            assert rc == EINVAL and "multiple of 32" in msg, (bad_c, msg)
        for bad_n in (0, -5):
            rc, msg = call(make(npix=bad_n))
            assert rc == EINVAL and "not positive" in msg, msg
        rc, msg = call(make(dtype=7))
        assert rc == EINVAL and "bad dtype" in msg, msg
    for alias in ("x", "a"):
        rc, msg = call(fwd(z=V(alias)))
        assert rc == EINVAL and "z aliases" in msg, msg
    for alias in ("x", "a", "z"):
        rc, msg = call(bwd(dx=V(alias)))
        assert rc == EINVAL and "dx aliases" in msg, msg
    for alias in ("x", "a", "dx"):
        rc, msg = call(bwd(da=V(alias)))
        assert rc == EINVAL and "da aliases" in msg, msg
    rc, msg = call(bwd(c=32, da=A.view(t["z"], c0=48)))                      # da overlaps dz without being dz
    assert rc == EINVAL and "da aliases" in msg, msg
    with pytest.raises(A.SrganfdError, match="multiple of 32"):
        ops.pixel_gate(fwd(c=16))


class _Calls:
    """stands in for the library handle: notes the name of every call that enqueues work, then makes it"""
    QUIET = ("srganfd_last_error", "srganfd_set_dry_run", "srganfd_abi_version", "srganfd_pack_layout", "srganfd_wgrad_plan_bytes",
             "srganfd_wgrad_plan_build", "srganfd_pack_weights", "srganfd_conv2d_describe")

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("srganfd_") or name in self.QUIET or "_workspace" in name:
            return fn

        def call(*args):
            self.names.append(name[len("srganfd_"):])
            return fn(*args)
        return call


# the documented sequences (sr_gan_fd_amd/engine_rpa.py); W = a weight-gradient launch, left out by a pass with frozen parameters
W = "conv2d_wgrad"
RPA_F = ["conv2d", "conv2d", "conv2d", "pixel_gate", "conv2d"]
US_F = ["conv2d", "conv2d", "pixel_gate", "conv2d"]
RPA_B = [W, "conv2d", "pixel_gate", W, "conv2d", W, "conv2d", W, "conv2d"]            # the last conv2d: the block input's gradient
US_B = [W, "conv2d", "resample", "pixel_gate", W, "conv2d", W, "conv2d"]


def sequences(kind, thin, n_rpa=1, n_us=1):
    if kind != "gen":
        f, b = (RPA_F, RPA_B) if kind == "rpa" else (US_F, US_B)
        return ["nchw_to_nhwc"] + f + ["nhwc_to_nchw"], ["nchw_to_nhwc", "lrelu_bwd"] + b + ["nhwc_to_nchw"]
    fwd = ["nchw_to_nhwc", "conv2d_thin_in" if thin else "conv2d"] + RPA_F * n_rpa + US_F * n_us + ["conv2d", "conv2d", "nhwc_to_nchw"]
    skip = ["lrelu_bwd"]                                                               # ds is complete: on to the last RPA
    bwd = ["nchw_to_nhwc", W, "conv2d", W, "conv2d"] + (US_B * n_us if n_us else []) + skip + RPA_B * n_rpa
    bwd += ["conv2d_thin_wgrad", "conv2d_thin_out"] if thin else [W, "conv2d"]
    return fwd, bwd + ["nhwc_to_nchw"]


@pytest.mark.parametrize("dt", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("kind,scale", [("rpa", 1), ("us", 2), ("gen", 1), ("gen", 2), ("gen", 4)])
def test_module_call_sequence(dry_run, kind, scale, dt):
    from sr_gan_fd_amd import model as M
    A = dry_run
    m = {"rpa": lambda: M.RPA(64), "us": lambda: M.US(64, 2), "gen": lambda: M.Generator_RPA(scale=scale, num_block=2)}[kind]()
    m.compute_dtype = dt
    n_us = len(m.us) if kind == "gen" else 1
    FORWARD, BACKWARD = sequences(kind, dt is torch.float16, 2, n_us)
    wgrads = ("conv2d_wgrad", "conv2d_thin_wgrad")
    rec = _Calls(A.lib())
    A._lib = rec
    try:
        x = torch.rand(2, 3 if kind == "gen" else 64, 5, 7, requires_grad=True)
        out = m(x)
        up = 1 if kind == "rpa" else 2 ** n_us
        assert out.shape == (2, x.shape[1], 5 * up, 7 * up) and out.dtype == torch.float32
        assert rec.names == FORWARD
        out.sum().backward()
        assert rec.names == FORWARD + BACKWARD
        assert x.grad.shape == x.shape and all(p.grad is not None and p.grad.shape == p.shape for p in m.parameters())
        del rec.names[:]
        with pytest.raises(A.SrganfdError, match="overwritten by a later forward"):      # the token check
            first = m(x)
            m(x)
            first.sum().backward()
        del rec.names[:]
        for p in m.parameters():                                # frozen parameters: no weight-gradient launches
            p.requires_grad_(False)
        m(x).sum().backward()
        assert rec.names == FORWARD + [n for n in BACKWARD if n not in wgrads]
        del rec.names[:]
        m(x.detach())                                           # nothing wants a gradient: the forward alone
        assert rec.names == FORWARD
        del rec.names[:]
        for p in m.parameters():                                # parameters only: the input's gradient is not computed
            p.requires_grad_(True)
        m(x.detach()).sum().backward()
        tail = 2 if kind != "gen" else 2                        # the first conv's data gradient and its layout conversion
        assert rec.names == FORWARD + BACKWARD[:-tail]
    finally:
        A._lib = rec._lib


def test_modules_refuse_what_has_no_kernel(dry_run):
    from sr_gan_fd_amd import model as M
    A = dry_run
    for bad in (lambda: M.RPA(16), lambda: M.US(48, 2), lambda: M.Generator_RPA(num_feat=32), lambda: M.Generator_RPA(num_feat=96, num_block=1)):
        with pytest.raises(A.SrganfdError, match="num_feat"):
            bad()
    with pytest.raises(A.SrganfdError, match="scale 3"):
        M.US(64, 3)(torch.randn(1, 64, 4, 4))
    with pytest.raises(A.SrganfdError, match="num_block"):
        M.Generator_RPA(num_block=0)(torch.rand(1, 3, 4, 4))
    with pytest.raises(A.SrganfdError, match=r"expects \(N, 64, H, W\)"):
        M.RPA(64)(torch.randn(1, 32, 4, 4))
    with pytest.raises(A.SrganfdError, match=r"expects \(N, 3, H, W\)"):
        M.Generator_RPA(num_block=1)(torch.randn(1, 4, 4, 4))
    m = M.RPA(64)
    m.compute_dtype = torch.float64
    with pytest.raises(A.SrganfdError, match="not supported"):
        m(torch.randn(1, 64, 4, 4))
    A.set_dry_run(False)
    for m, c in ((M.RPA(64), 64), (M.US(64, 2), 64), (M.Generator_RPA(num_block=1), 3)):
        with pytest.raises(A.SrganfdError, match="not on a GPU"):
            m(torch.randn(1, c, 4, 4))


def test_compute_dtype_pins_the_precision(dry_run):
    from sr_gan_fd_amd import model as M
    from sr_gan_fd_amd.engine_rpa import rpa_engine
    A = dry_run
    m = M.RPA(64)
    x = torch.randn(1, 64, 3, 4)
    m(x)
    assert rpa_engine(m, "rpa")._last.dtc == A.F32
    for dt, code in ((torch.float16, A.F16), (torch.bfloat16, A.BF16)):
        m.compute_dtype = dt
        m(x)
        assert rpa_engine(m, "rpa")._last.dtc == code


def test_launch_item_has_label_and_bytes():
    from sr_gan_fd_amd import _abi as A, ops
    t = torch.zeros(10, 64)
    f = ops.PixelGate(ops.pixel_gate_args(A.F16, 10, 64, A.view(t), A.view(t), z=A.view(t)))
    b = ops.PixelGate(ops.pixel_gate_args(A.F32, 10, 64, A.view(t), A.view(t), dz=A.view(t), dx=A.view(t), da=A.view(t)))
    assert (f.kind, f.label, f.work) == ("pixel_gate", "pixel_gate_fwd_kernel<f16>", (0.0, 10 * 64 * 2 * 3.0))
    assert (b.kind, b.label, b.work) == ("pixel_gate", "pixel_gate_bwd_kernel<f32>", (0.0, 10 * 64 * 4 * 5.0))
