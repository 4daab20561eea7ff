"""CPU-only host-logic tests: the C ABI loads and exports every declared symbol, argument validation
works, and the engines' launch plans (views, channel slices, shapes, workspaces) are self-consistent.
Kernels are NOT executed here (library dry-run mode): numerics are covered by the -m gpu tests."""
import ctypes as C
import re
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_header_symbol():
    from sr_gan_fd_amd import _abi as A
    hdr = open(os.path.join(ROOT, "include", "srganfd.h")).read()
    # declarations inside `#ifdef SRGANFD_EXPERIMENT` belong to the timing-experiment builds only (tools/build_variant.sh)
    experiment = re.findall(r"#ifdef SRGANFD_EXPERIMENT(.*?)#endif", hdr, re.S)
    product_hdr = re.sub(r"#ifdef SRGANFD_EXPERIMENT.*?#endif", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(srganfd_[a-z0-9_]+)\s*\(", product_hdr))
    lib = C.CDLL(A.LIB_PATH)
    for name in re.findall(r"\b(srganfd_[a-z0-9_]+)\s*\(", " ".join(experiment)):
        assert not hasattr(lib, name), f"{name} (experiment hook) must not be exported by the product library"
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/srganfd.h but not exported"
    assert declared == set(A.SYMBOLS), f"binding/header mismatch: {declared ^ set(A.SYMBOLS)}"
    assert A.lib().srganfd_abi_version() == A.ABI_VERSION == A._ABI_VERSION_BUILT == 7
    assert A.lib().srganfd_get_mfma16() == 3


_BINDING_CHECK_PRELUDE = r"""
#include <stddef.h>
#include <stdint.h>
#include "srganfd.h"
// one class letter per argument / return type; a type outside this table has no K<> and fails to compile
template <class T> struct K;
template <> struct K<void> { static constexpr char c = 'v'; };
template <> struct K<int32_t> { static constexpr char c = 'i'; };
template <> struct K<int64_t> { static constexpr char c = 'l'; };
template <> struct K<size_t> { static constexpr char c = 'z'; };
template <> struct K<float> { static constexpr char c = 'f'; };
template <> struct K<double> { static constexpr char c = 'd'; };
template <> struct K<srganfd_view> { static constexpr char c = 'V'; };
template <class T> struct K<T*> { static constexpr char c = 'p'; };
template <class F> struct Sig;
template <class R, class... A> struct Sig<R (*)(A...)> { static constexpr char s[sizeof...(A) + 2] = {K<R>::c, K<A>::c..., 0}; };
constexpr bool eq(const char* a, const char* b) { return *a == *b && (*a == 0 || eq(a + 1, b + 1)); }
"""


def _ctype_class(t) -> str:
    from sr_gan_fd_amd import _abi as A
    if t is None:
        return "v"
    if t is A.View:
        return "V"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return "p"
    return {C.c_int32: "i", C.c_int64: "l", C.c_size_t: "z", C.c_float: "f", C.c_double: "d"}[t]   # c_int is c_int32; anything else: KeyError


def binding_check_source(A) -> str:
    """A translation unit of static_asserts that holds sr_gan_fd_amd/_abi.py against include/srganfd.h: every SYMBOLS entry's return and
    argument classes, every Structure's size and its fields' offsets and sizes, and the constants the binding repeats."""
    out = [_BINDING_CHECK_PRELUDE]
    for name, (res, args) in A.SYMBOLS.items():
        sig = _ctype_class(res) + "".join(_ctype_class(a) for a in args)
        out.append(f'static_assert(eq(Sig<decltype(&{name})>::s, "{sig}"), "{name}");')
    structs = [v for v in vars(A).values() if isinstance(v, type) and issubclass(v, C.Structure) and v.__module__ == A.__name__]
    assert structs and all("C_NAME" in vars(s) for s in structs), "every Structure of _abi.py names the C struct it mirrors (C_NAME)"
    for s in structs:
        out.append(f'static_assert(sizeof({s.C_NAME}) == {C.sizeof(s)}, "sizeof({s.C_NAME}) != sizeof({s.__name__})");')
        for field, _ in s._fields_:
            d = getattr(s, field)
            out.append(f'static_assert(offsetof({s.C_NAME}, {field}) == {d.offset} && sizeof({s.C_NAME}::{field}) == {d.size}, '
                       f'"{s.C_NAME}.{field} vs {s.__name__}.{field}");')
    consts = {"SRGANFD_BF16": A.BF16, "SRGANFD_F32": A.F32, "SRGANFD_F16": A.F16, "SRGANFD_ACT_NONE": A.ACT_NONE, "SRGANFD_ACT_LRELU": A.ACT_LRELU,
              "SRGANFD_ACT_RELU": A.ACT_RELU, "SRGANFD_LOSS_WS_FLOATS": A.LOSS_WS_FLOATS, "SRGANFD_ABI_VERSION": A._ABI_VERSION_BUILT}
    for cname, val in consts.items():
        out.append(f'static_assert({cname} == {val}, "{cname} is not the binding\'s {val}");')
    return "\n".join(out) + "\n"


def _cxx_compiler():
    import shutil
    rocm = os.environ.get("ROCM_PATH") or "/opt/rocm"
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++", os.path.join(rocm, "llvm", "bin", "clang++")):
        if c and shutil.which(c.split()[0]):
            return c.split()
    return None


def test_binding_matches_header(tmp_path):
    """The ctypes binding is compiled against the header: a wrong width, a misplaced argument, a field out of order or a stale constant
    in _abi.py is a failed static_assert that names the symbol or field.  No GPU and no built library are needed."""
    import subprocess
    from sr_gan_fd_amd import _abi as A
    cxx = _cxx_compiler()
    if cxx is None:
        pytest.skip("no C++ compiler found ($CXX, c++, g++, clang++, ROCm's clang++)")
    src = tmp_path / "binding_check.cpp"
    src.write_text(binding_check_source(A))
    r = subprocess.run(cxx + ["-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, "sr_gan_fd_amd/_abi.py disagrees with include/srganfd.h:\n" + r.stderr[-4000:]


def test_product_path_fails_loudly_without_gpu():
    from sr_gan_fd_amd import _abi as A, model as M
    net = M.bsrgan_x4(num_rrdb=1)
    with pytest.raises(A.SrganfdError):
        net(torch.rand(1, 3, 8, 8))


def test_conv_argument_validation():
    from sr_gan_fd_amd import _abi as A, ops
    A.set_dry_run(True)
    try:
        x = torch.zeros(1, 8, 8, 64)
        y = torch.zeros(1, 8, 8, 32)
        w = torch.zeros(64 * 32 * 9 * 2, dtype=torch.uint8)
        ok = ops.conv_args(A.BF16, A.view(x), A.view(y), w, 1, 8, 8, 64, 32)
        ops.conv2d(ok)
        bad = ops.conv_args(A.BF16, A.view(x), A.view(y), w, 1, 8, 8, 48, 32)   # cin not a multiple of 32
        with pytest.raises(A.SrganfdError):
            ops.conv2d(bad)
        bad = ops.conv_args(A.BF16, A.view(x, c0=40), A.view(y), w, 1, 8, 8, 64, 32)  # view exceeds buffer
        with pytest.raises(A.SrganfdError):
            ops.conv2d(bad)
        bad = ops.conv_args(A.BF16, A.view(x), A.view(y), w, 1, 8, 8, 64, 32)
        bad.h_out = 9
        with pytest.raises(A.SrganfdError):
            ops.conv2d(bad)
    finally:
        A.set_dry_run(False)


@pytest.mark.parametrize("fac,kw", [("bsrgan_x4", dict(num_rrdb=2)), ("bsrgan_x2", dict(num_rrdb=1)),
                                    ("rrdbnet_x1", dict(num_blocks=1)), ("rrdbnet_x8", dict(num_blocks=1))])
def test_generator_plan_dry_run(fac, kw):
    """forward + backward launch lists validate against the C ABI's shape checks (no kernels run)"""
    from sr_gan_fd_amd import _abi as A, model as M
    A.set_dry_run(True)
    try:
        net = getattr(M, fac)(**kw)
        for dt in (torch.float32, torch.bfloat16):
            net.compute_dtype = dt
            x = torch.rand(2, 3, 12, 20)
            sr = net(x)
            s = net.upscale_factor if fac.startswith("rrdb") else max(net.upscale_factor, 2)
            assert sr.shape == (2, 3, 12 * s, 20 * s)
            sr.sum().backward()
            for n, p in net.named_parameters():
                assert p.grad is not None and p.grad.shape == p.shape, n
            net.zero_grad(set_to_none=True)
            with torch.no_grad():
                assert net(x).shape == sr.shape
    finally:
        A.set_dry_run(False)


def test_flat_params_alias_module_parameters():
    from sr_gan_fd_amd import _abi as A, model as M, engine as E
    A.set_dry_run(True)
    try:
        net = M.bsrgan_x4(num_rrdb=1)
        sd0 = {k: v.clone() for k, v in net.state_dict().items()}
        net(torch.rand(1, 3, 8, 8))
        eng = E.generator_engine(net)
        flat = eng.fp.flat
        for (n, p), o in zip(net.named_parameters(), eng.fp.offsets):
            assert p.data_ptr() == flat.data_ptr() + 4 * o
            assert torch.equal(p.detach(), sd0[n]), n        # flattening must not change values
        assert list(net.state_dict().keys()) == list(sd0.keys())
    finally:
        A.set_dry_run(False)


@pytest.mark.parametrize("which", ["unet", "aesrgan", "esrgan"])
def test_discriminator_plans_dry_run(which):
    """the three discriminators' forward / backward launch lists pass the C ABI's argument checks (no kernels run)"""
    from sr_gan_fd_amd import _abi as A, model as M
    A.set_dry_run(True)
    try:
        d = {"unet": lambda: M.discriminator_unet(in_channels=3, out_channels=1, channels=64), "aesrgan": M.uNetDiscriminatorAesrgan,
             "esrgan": M.discriminator}[which]()
        size = 128 if which == "esrgan" else 64
        for dt in (torch.float32, torch.bfloat16):
            d.compute_dtype = dt
            d.train()
            x = torch.rand(2, 3, size, size, requires_grad=True)
            out = d(x)
            assert out.shape == ((2, 1) if which == "esrgan" else (2, 1, size, size))
            out.sum().backward()
            assert x.grad is not None and x.grad.shape == x.shape
            for n, p in d.named_parameters():
                assert p.grad is not None and p.grad.shape == p.shape, n
            d.zero_grad(set_to_none=True)
        if which == "esrgan":
            with pytest.raises(A.SrganfdError):
                d(torch.rand(1, 3, 64, 64))            # the classifier fixes the input size (ESRGAN/model.py:129)
    finally:
        A.set_dry_run(False)


def test_content_losses_and_fused_trainers_dry_run():
    from sr_gan_fd_amd import _abi as A, model as M
    from sr_gan_fd_amd.gan import GanTrainer
    from sr_gan_fd_amd.trainer import GeneratorTrainer
    nodes, mean, std = ["features.2", "features.7", "features.16", "features.25", "features.34"], [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    A.set_dry_run(True)
    try:
        cl5 = M.ContentLoss(nodes, mean, std)
        cl1 = M.ContentLoss("features.34", mean, std)
        sr = torch.rand(2, 3, 32, 48, requires_grad=True)
        gt = torch.rand(2, 3, 32, 48)
        v5 = cl5(sr, gt)
        assert v5.shape == (1, 5) and not v5.requires_grad           # detached like torch.Tensor([losses]) (model.py:552)
        v1 = cl1(sr, gt)
        assert v1.dim() == 0 and v1.requires_grad                    # ESRGAN's stays in the graph
        v1.backward()
        assert sr.grad.shape == sr.shape
        with pytest.raises(A.SrganfdError):
            cl1(torch.rand(1, 3, 30, 32), torch.rand(1, 3, 30, 32))   # four 2x2 pools
        g = M.bsrgan_x4(num_rrdb=1)
        assert g.compute_dtype is None
        t = GeneratorTrainer(g, lr=1e-4)
        # a trainer built over default modules, outside autocast, trains as the reference's loop does:
        # float16 with the loss scaler on -- not in the exact-fp32 parity mode the modules run in outside autocast
        assert g.compute_dtype == torch.float16 and t.scaler.enabled
        assert t.step(torch.rand(2, 3, 16, 16), torch.rand(2, 3, 64, 64)).shape == (1,)
        for dfac in (lambda: M.discriminator_unet(in_channels=3, out_channels=1, channels=64), M.uNetDiscriminatorAesrgan):
            tr = GanTrainer(M.bsrgan_x4(num_rrdb=1), dfac(), M.ContentLoss(nodes, mean, std))
            assert tr.g.compute_dtype == tr.d.compute_dtype == tr.content.compute_dtype == torch.float16 and tr.scaler.enabled
            assert tr.step(torch.rand(2, 3, 16, 16), torch.rand(2, 3, 64, 64)).shape == (8,)
            assert tr.content_vals.shape == (1, 5)
        # an explicit dtype is kept (the parity tests' float32, configs[0]), and a bfloat16 autocast region is followed
        g32 = M.bsrgan_x4(num_rrdb=1)
        g32.compute_dtype = torch.float32
        assert not GeneratorTrainer(g32, lr=1e-4).scaler.enabled and g32.compute_dtype == torch.float32
        if torch.cuda.is_available():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                gb = M.bsrgan_x4(num_rrdb=1)
                assert not GeneratorTrainer(gb, lr=1e-4).scaler.enabled and gb.compute_dtype == torch.bfloat16
    finally:
        A.set_dry_run(False)


def test_planar_views_are_validated():
    """srganfd_view.planar (32-channel group planes): conv2d / conv2d_wgrad accept it for aligned channel ranges only"""
    from sr_gan_fd_amd import _abi as A, ops
    A.set_dry_run(True)
    try:
        L = A.lib()
        x = torch.zeros(1, 8, 8, 192)
        y = torch.zeros(1, 8, 8, 192)
        wp = torch.zeros(ops.packed_bytes(A.BF16, 3, 96, 32), dtype=torch.uint8)
        ok = ops.conv_args(A.BF16, A.view(x, planar=1), A.view(y, c0=96, planar=1), wp.data_ptr(), 1, 8, 8, 96, 32)
        assert L.srganfd_conv2d(C.byref(ok), None) == 0
        bad = ops.conv_args(A.BF16, A.view(x, planar=1), A.view(y, c0=104, planar=1), wp.data_ptr(), 1, 8, 8, 96, 32)
        assert L.srganfd_conv2d(C.byref(bad), None) != 0 and b"planar" in L.srganfd_last_error()
        f32out = ops.conv_args(A.BF16, A.view(x, planar=1), A.view(torch.zeros(1, 8, 8, 32), planar=1), wp.data_ptr(), 1, 8, 8, 96, 32, y_f32=True)
        assert L.srganfd_conv2d(C.byref(f32out), None) != 0
    finally:
        A.set_dry_run(False)


def test_resampling_and_layout_entry_points_refuse_planar_views_and_bad_arguments():
    """include/srganfd.h: only the convolutions take planar views.  Every other entry point read one as NHWC without a word."""
    from sr_gan_fd_amd import _abi as A
    L = A.lib()
    A.set_dry_run(True)
    try:
        p = 4096                                              # a non-null, 16-byte aligned address; nothing is dereferenced in dry-run mode
        V = lambda planar=0, cs=64, c0=0: A.View(p, cs, c0, planar, 0)
        calls = {
            "resample a": lambda a, b: L.srganfd_resample(1, a, b, A.F16, 2, 4, 4, 32, 0),
            "resample_bwd_lrelu": lambda a, b: L.srganfd_resample_bwd_lrelu(a, b, V(), V(), A.F16, 2, 4, 4, 32, 0.2, 0),
            "resample_bwd_lrelu act": lambda a, b: L.srganfd_resample_bwd_lrelu(V(), V(), a, b, A.F16, 2, 4, 4, 32, 0.2, 0),
            "resize_bilinear": lambda a, b: L.srganfd_resize_bilinear(0, a, b, A.F16, 2, 4, 4, 8, 8, 32, 0),
            "maxpool2_relu_bwd": lambda a, b: L.srganfd_maxpool2_relu_bwd(a, b, V(), A.F16, 2, 4, 4, 32, 0),
            "maxpool2_relu_bwd dx": lambda a, b: L.srganfd_maxpool2_relu_bwd(V(), a, b, A.F16, 2, 4, 4, 32, 0),
            "clamp_grad": lambda a, b: L.srganfd_clamp_grad_to_nhwc(p, a, 2, 3, 4, 4, b, A.F16, 32, 0),
        }
        one_view = {
            "nchw_to_nhwc": lambda v: L.srganfd_nchw_to_nhwc(p, 2, 3, 4, 4, v, A.F16, 32, None, None, 0),
            "nhwc_to_nchw": lambda v: L.srganfd_nhwc_to_nchw(v, A.F16, 2, 3, 4, 4, p, 1, 0),
            "nhwc_to_nchw_scaled": lambda v: L.srganfd_nhwc_to_nchw_scaled(v, 2, 3, 4, 4, p, p, 0),
        }
        for name, f in calls.items():
            assert f(V(), V()) == 0, name + ": " + L.srganfd_last_error().decode()
            for a, b in ((V(1), V()), (V(), V(1))):
                assert f(a, b) == -1 and b"planar" in L.srganfd_last_error(), name
        for name, f in one_view.items():
            assert f(V()) == 0, name + ": " + L.srganfd_last_error().decode()
            assert f(V(1)) == -1 and b"planar" in L.srganfd_last_error(), name
        # channels past the buffer's, an operation there is not
        assert L.srganfd_resample(1, V(c0=40), V(), A.F16, 2, 4, 4, 32, 0) == -1 and L.srganfd_resample(1, V(), V(c0=40), A.F16, 2, 4, 4, 32, 0) == -1
        for vec in (V(), V(c0=4)):                            # the vector and the scalar forms' dispatch
            assert L.srganfd_resample(5, vec, V(), A.F16, 2, 4, 4, 32, 0) == -1 and b"bad op" in L.srganfd_last_error()
            assert L.srganfd_resample(-1, vec, V(), A.F16, 2, 4, 4, 32, 0) == -1
            assert all(L.srganfd_resample(op, vec, V(), A.F16, 2, 4, 4, 32, 0) == 0 for op in range(5))
    finally:
        A.set_dry_run(False)


def test_elementwise_loss_and_adam_entry_points_refuse_planar_views_bad_slices_and_bad_counts():
    """include/srganfd.h: only the convolutions take planar views.  The per-element maps, the L1 losses on views, the attention gate's
    pieces and BatchNorm read one as NHWC without a word, took a slice that ends past its buffer, and turned a negative count into a
    grid over 2^64 elements.  Dry run with made-up addresses: nothing of this may ever reach a GPU."""
    from sr_gan_fd_amd import _abi as A
    L = A.lib()
    A.set_dry_run(True)
    try:
        p = 4096                                              # a non-null, 16-byte aligned address; nothing is dereferenced in dry-run mode
        V = lambda planar=0, cs=64, c0=0: A.View(p, cs, c0, planar, 0)
        err = lambda: L.srganfd_last_error()
        wrong = []                                            # every case is tried, so that a failure lists all of them

        def expect(ok, what):
            if not ok:
                wrong.append(str(what))

        bn_fwd = lambda x, y: (x, y, A.F16, 64, 32, p, p, p, p, 0.1, 1e-5)
        bn_bwd = lambda x, dy, dx: (x, dy, dx, A.F16, 64, 32, p, p, p, p, 0.0, p)
        # every view argument of every entry point in turn: (name, number of views, call(views, npix, c))
        on_views = [
            ("lrelu_bwd", 4, lambda v, n, c: L.srganfd_lrelu_bwd(v[0], v[1], v[2], v[3], A.F16, n, c, 0.2, 0)),
            ("lrelu_bwd scalar form", 4, lambda v, n, c: L.srganfd_lrelu_bwd(v[0], v[1], v[2], v[3], A.F32, n, c - 1 if c > 1 else c, 0.2, 0)),
            ("axpby", 2, lambda v, n, c: L.srganfd_axpby(v[0], v[1], A.F16, n, c, 1.0, 1.0, 0)),
            ("axpby scalar form", 2, lambda v, n, c: L.srganfd_axpby(v[0], v[1], A.F32, n, c - 1 if c > 1 else c, 1.0, 0.0, 0)),
            ("add_relu", 3, lambda v, n, c: L.srganfd_add_relu(v[0], v[1], v[2], A.F16, n, c, 0)),
            ("gate_mul", 2, lambda v, n, c: L.srganfd_gate_mul(0, v[0], p, v[1], A.NULL_VIEW, None, A.F16, n, c, 0)),
            ("gate_mul bwd", 3, lambda v, n, c: L.srganfd_gate_mul(1, v[0], p, v[1], v[2], p, A.F16, n, c, 0)),
            ("l1_loss_views", 2, lambda v, n, c: L.srganfd_l1_loss_views(v[0], v[1], A.F16, n, c, 1, 1.0, p, 0, p, 0)),
            ("l1_loss_views scalar form", 2, lambda v, n, c: L.srganfd_l1_loss_views(v[0], v[1], A.F32, n, c - 1 if c > 1 else c, 0, 1.0, p, 0, p, 0)),
            ("l1_grad_views", 3, lambda v, n, c: L.srganfd_l1_grad_views(v[0], v[1], v[2], A.F16, n, c, None, 1.0, 0)),
        ]
        for name, nv, f in on_views:
            good = [V() for _ in range(nv)]
            expect(f(good, 6, 32) == 0, name + ": " + err().decode())
            for k in range(nv):
                expect(f(good[:k] + [V(1)] + good[k + 1:], 6, 32) == -1 and b"planar" in err(), f"{name}: planar view {k}")
                expect(f(good[:k] + [V(c0=40)] + good[k + 1:], 6, 32) == -1 and b"past its buffer" in err(), f"{name}: view {k} ends past its buffer")
                expect(f(good[:k] + [V(c0=32)] + good[k + 1:], 6, 32) == 0, f"{name}: view {k} ends with its buffer: " + err().decode())
            for n in (-1, -2 ** 40, 0):
                expect(f(good, n, 32) == -1 and b"npix <= 0" in err(), f"{name}: npix = {n}")
            for c in (0, -8):
                expect(f(good, 6, c) == -1, f"{name}: c = {c}")
        expect(L.srganfd_lrelu_bwd(V(), V(), V(), V(), A.F16, 6, 0, 0.2, 0) == -1 and b"c <= 0" in err(), "lrelu_bwd: c = 0 names its cause")
        expect(L.srganfd_axpby(V(), V(), A.F16, 6, 0, 1.0, 1.0, 0) == -1 and b"c <= 0" in err(), "axpby: c = 0 names its cause")
        expect(L.srganfd_l1_loss_views(V(), V(), A.F16, 6, 0, 0, 1.0, p, 0, p, 0) == -1 and b"c <= 0" in err(), "l1_loss_views: c = 0 names its cause")
        # the flat single-channel form the trainers add gradients with
        expect(L.srganfd_axpby(A.View(p, 1, 0), A.View(p + 64, 1, 0), A.F32, 1000, 1, 1.0, 1.0, 0) == 0, "axpby: the flat form")
        # BatchNorm, all six forms: planar, and a slice past its buffer, on every view (act included)
        bn = [
            ("batchnorm_fwd", 2, lambda v: L.srganfd_batchnorm_fwd(*bn_fwd(v[0], v[1]), 1, p, p, 0)),
            ("batchnorm_act_fwd", 2, lambda v: L.srganfd_batchnorm_act_fwd(*bn_fwd(v[0], v[1]), 1, p, p, 0.2, 0)),
            ("batchnorm_fwd_sync", 2, lambda v: L.srganfd_batchnorm_fwd_sync(*bn_fwd(v[0], v[1]), p, p, 0.2, 1, 0, 0)),
            ("batchnorm_bwd", 3, lambda v: L.srganfd_batchnorm_bwd(*bn_bwd(v[0], v[1], v[2]), 0)),
            ("batchnorm_act_bwd", 4, lambda v: L.srganfd_batchnorm_act_bwd(*bn_bwd(v[0], v[1], v[2]), v[3], 0.2, 0)),
            ("batchnorm_bwd_sync", 4, lambda v: L.srganfd_batchnorm_bwd_sync(*bn_bwd(v[0], v[1], v[2]), None, v[3], 0.2, 1, 0, 0)),
        ]
        for name, nv, f in bn:
            good = [V() for _ in range(nv)]
            expect(f(good) == 0, name + ": " + err().decode())
            for k in range(nv):
                expect(f(good[:k] + [V(1)] + good[k + 1:]) == -1 and b"planar" in err(), f"{name}: planar view {k}")
                expect(f(good[:k] + [V(c0=40)] + good[k + 1:]) == -1 and b"past its buffer" in err(), f"{name}: view {k} ends past its buffer")
        # flat arrays: a count that is negative or zero
        ws = p
        flat = {
            "l1_loss": lambda n: L.srganfd_l1_loss(p, p, n, 1.0, p, 0, p, 1.0, None, ws, 0),
            "bce_logits": lambda n: L.srganfd_bce_logits(p, n, 1.0, 1.0, p, 0, p, p, 1.0, None, ws, 0),
            "nonfinite_flag": lambda n: L.srganfd_nonfinite_flag(p, n, p, 0, 0),
            "adam_ema": lambda n: L.srganfd_adam_ema(p, p, p, p, p, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, 0.999, 2, None, None, 0),
            "adam_ema_dev": lambda n: L.srganfd_adam_ema_dev(p, p, p, p, p, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, p, p, 1.0, 0.999, 2, None, None, 0),
            "sigmoid": lambda n: L.srganfd_sigmoid(p, n, 0),
            "sigmoid_bwd": lambda n: L.srganfd_sigmoid_bwd(p, p, p, n, 0),
            "sigmoid_of_mean": lambda n: L.srganfd_sigmoid_of_mean(p, n, p, ws, 0),
            "bce_logits_relativistic": lambda n: L.srganfd_bce_logits_relativistic(p, n, p, 5, 1.0, 1.0, p, 0, p, 0, p, 0, 1.0, None, ws, 0),
            "bce_logits_relativistic other": lambda n: L.srganfd_bce_logits_relativistic(p, 5, p, n, 1.0, 1.0, p, 0, p, 0, p, 0, 1.0, None, ws, 0),
        }
        for name, f in flat.items():
            expect(f(1000) == 0 and f(1) == 0, name + ": " + err().decode())
            for n in (-1, -2 ** 40, 0):
                expect(f(n) == -1, f"{name}: numel = {n}")
                if "relativistic" not in name and name != "sigmoid_of_mean":
                    expect(b"numel <= 0" in err(), f"{name}: numel = {n}: {err().decode()}")
        # Adam's EMA mode
        for mode, rc in ((0, 0), (1, 0), (2, 0), (3, -1), (-1, -1)):
            expect(L.srganfd_adam_ema(p, p, p, p, p, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, 0.999, mode, None, None, 0) == rc and (rc == 0 or b"ema_mode" in err()), f"adam: ema_mode = {mode}")
            expect(L.srganfd_adam_ema_dev(p, p, p, p, p, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, p, p, 1.0, 0.999, mode, None, None, 0) == rc and (rc == 0 or b"ema_mode" in err()), f"adam: ema_mode = {mode}")
        assert not wrong, "%d cases:\n  " % len(wrong) + "\n  ".join(wrong)
    finally:
        A.set_dry_run(False)


def test_validation_side_argument_checks():
    from sr_gan_fd_amd import _abi as A
    A.set_dry_run(True)
    try:
        L = A.lib()
        buf = torch.zeros(64)
        p = buf.data_ptr()
        assert L.srganfd_crop_nchw(p, p, 1, 3, 8, 8, 2, 2, 4, 4, None) == 0
        assert L.srganfd_crop_nchw(p, p, 1, 3, 8, 8, 6, 2, 4, 4, None) != 0          # window leaves the image
        assert L.srganfd_psnr(p, p, 1, 3, 8, 8, 2, 1, p, p, None) == 0
        assert L.srganfd_psnr(p, p, 1, 1, 8, 8, 2, 1, p, p, None) != 0              # luma needs RGB
        assert L.srganfd_psnr(p, p, 1, 3, 8, 8, 4, 0, p, p, None) != 0              # nothing left after the crop
        assert L.srganfd_ssim_workspace_doubles(2, 3, 40, 56, 4, 1, 11) == 2 * 1 * 2 * 3   # 22x38 map -> 2x3 tiles of 16x16
        assert L.srganfd_ssim_workspace_doubles(2, 3, 40, 56, 4, 0, 11) == 2 * 3 * 2 * 3
        assert L.srganfd_ssim_workspace_doubles(1, 3, 12, 12, 1, 1, 11) == 0               # window larger than the cropped image
        assert L.srganfd_ssim(p, p, 1, 3, 16, 16, 2, 1, p, 11, p, p, None) == 0
        assert L.srganfd_ssim(p, p, 1, 3, 12, 12, 1, 1, p, 11, p, p, None) != 0            # window does not fit
        assert L.srganfd_ssim(p, p, 1, 1, 16, 16, 0, 1, p, 11, p, p, None) != 0            # luma needs RGB
        assert L.srganfd_ssim(p, p, 1, 3, 32, 32, 0, 0, p, 17, p, p, None) != 0            # window above the kernel's LDS tile
        # on-device degradation stages (Real_ESRGAN/imgproc.py)
        assert L.srganfd_filter2d(p, p, 1, 2, 3, 32, 32, 21, p, None) == 0
        assert L.srganfd_filter2d(p, p, 2, 2, 3, 32, 32, 21, p, None) == 0
        assert L.srganfd_filter2d(p, p, 1, 2, 3, 32, 32, 4, p, None) != 0 and b"Wrong kernel size." in L.srganfd_last_error()
        assert L.srganfd_filter2d(p, p, 3, 2, 3, 32, 32, 21, p, None) != 0                   # 3 kernels for 2 images
        assert L.srganfd_filter2d(p, p, 1, 2, 3, 10, 32, 21, p, None) != 0                   # reflect padding 10 needs > 10 rows
        assert L.srganfd_filter2d(p, p, 1, 2, 3, 64, 64, 53, p, None) != 0                   # above the LDS tile
        assert L.srganfd_filter2d_separable(p, p, 1, 2, 3, 64, 64, 51, p, None) == 0
        assert L.srganfd_usm_sharp(p, p, 0, 1, 3, 64, 64, 51, 0.5, 10.0, p, p, None) == 0 and L.srganfd_usm_sharp(p, p, 1, 1, 3, 64, 64, 51, 0.5, 10.0, p, p, None) == 0
        assert L.srganfd_usm_sharp(p, p, 0, 1, 3, 64, 64, 51, 0.5, 10.0, p, None, None) != 0    # workspace required
        assert L.srganfd_diff_jpeg_table_floats() == 2 * 4096 + 4 * 64
        assert L.srganfd_diff_jpeg(p, 2, 3, 17, 33, p, 0, 0, p, p, None) == 0
        assert L.srganfd_diff_jpeg(p, 2, 1, 16, 16, p, 0, 0, p, p, None) != 0                # RGB only
        assert L.srganfd_resize(p, 6, 32, 32, 8, 8, 0, 0.0, 0.0, p, None) == 0
        assert L.srganfd_resize(p, 6, 32, 32, 8, 8, 3, 0.0, 0.0, p, None) != 0               # unknown mode
        assert L.srganfd_resize(p, 6, 32, 32, 0, 8, 1, 0.0, 0.0, p, None) != 0
        assert L.srganfd_gaussian_noise(p, p, None, p, None, 2, 3, 8, 8, 1, 0, p, None) == 0
        assert L.srganfd_gaussian_noise(p, p, p, p, None, 2, 3, 8, 8, 1, 0, p, None) != 0    # grey field without the grey flags
        assert L.srganfd_poisson_prepare(p, 2, 3, 8, 8, 0, p, None, p, None, p, None) == 0
        assert L.srganfd_poisson_prepare(p, 2, 1, 8, 8, 1, p, p, p, p, p, None) != 0         # grey needs RGB
        assert L.srganfd_poisson_apply(p, p, None, p, None, p, None, p, None, 2, 3, 8, 8, 1, 0, p, None) == 0
        assert L.srganfd_poisson_apply(p, p, None, p, p, p, None, p, None, 2, 3, 8, 8, 1, 0, p, None) != 0
        assert L.srganfd_quantize_u8(p, p, 64, None) == 0 and L.srganfd_quantize_u8(p, p, 0, None) != 0
        assert L.srganfd_crop_rot_flip(p, p, 6, 8, 8, 2, 2, 4, 4, 1, None) == 0
        assert L.srganfd_crop_rot_flip(p, p, 6, 8, 8, 2, 2, 4, 6, 1, None) != 0              # quarter turn of a non-square window
        assert L.srganfd_crop_rot_flip(p, p, 6, 8, 8, 6, 2, 4, 4, 0, None) != 0              # window leaves the image
        assert L.srganfd_crop_rot_flip(p, p, 6, 8, 8, 0, 0, 8, 8, 6, None) != 0              # unknown op
    finally:
        A.set_dry_run(False)


def test_diff_jpeg_tables_are_the_oracles_standard_tables_transposed():
    """csrc/jpeg.hip keeps one copy of the standard quantisation tables for both round trips: what srganfd_diff_jpeg_tables derives from it
    for DiffJPEG (the reference transposes them) is tests/jpeg_oracle.py's copy, which the integer round trip is tested against"""
    import numpy as np
    from sr_gan_fd_amd import _abi as A
    from tests import jpeg_oracle as JO
    A.set_dry_run(True)
    try:
        L = A.lib()
        t = np.zeros(L.srganfd_diff_jpeg_table_floats(), dtype=np.float32)
        assert L.srganfd_diff_jpeg_tables(t.ctypes.data) == 0
        y, c = t[8192 + 128:8192 + 192].reshape(8, 8), t[8192 + 192:8192 + 256].reshape(8, 8)
        assert np.array_equal(y, JO.LUMA.T.astype(np.float32)) and np.array_equal(c, JO.CHROMA.T.astype(np.float32))
        assert L.srganfd_diff_jpeg_tables(None) != 0
    finally:
        A.set_dry_run(False)


def test_modules_deepcopy_and_pickle_like_the_train_scripts_do():
    """AveragedModel deep-copies the generator (train_bsrgan.py:291) and mlflow.pytorch.log_model pickles both networks
    (:203-213): copies must carry the same state_dict, own their parameters, and still run"""
    import copy
    import pickle
    from sr_gan_fd_amd import _abi as A, model as M
    A.set_dry_run(True)
    try:
        nodes, mean, std = ["features.2", "features.34"], [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
        mods = [M.bsrgan_x4(num_rrdb=1), M.rrdbnet_x4(num_blocks=1), M.discriminator_unet(in_channels=3, out_channels=1, channels=64),
                M.uNetDiscriminatorAesrgan(), M.discriminator(), M.ContentLoss(nodes, mean, std)]
        for m in mods:
            if not isinstance(m, M.ContentLoss):
                m(torch.rand(1, 3, 128, 128) if isinstance(m, M.Discriminator) else torch.rand(1, 3, 64, 64))   # build the engine first
            for clone in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
                assert type(clone) is type(m)
                sd, sc = m.state_dict(), clone.state_dict()
                assert list(sd) == list(sc) and all(torch.equal(sd[k], sc[k]) for k in sd)
                p0, c0 = next(m.parameters()), next(clone.parameters())
                assert p0.data_ptr() != c0.data_ptr()
                with torch.no_grad():
                    c0.add_(1.0)
                assert not torch.equal(p0, c0)                       # no aliasing of the flat parameter buffers
                if isinstance(m, M.ContentLoss):
                    assert clone(torch.rand(1, 3, 32, 32), torch.rand(1, 3, 32, 32)).shape == (1, 2)
                elif isinstance(m, M.Discriminator):
                    assert clone(torch.rand(1, 3, 128, 128)).shape == (1, 1)
                else:
                    clone(torch.rand(1, 3, 64, 64))
    finally:
        A.set_dry_run(False)


def test_engines_release_their_buffers_by_reference_counting():
    """A plan closure that captures its engine or its own plan object is a reference cycle: the activation buffers (hundreds of
    GB at the benchmark sizes) then outlive the module until a cyclic collection that HIP allocations never trigger -- an
    out-of-memory error between two full-size tests.  After dropping the modules, the cyclic collector must find no tensor
    and no engine."""
    import gc
    from sr_gan_fd_amd import _abi as A, model as M
    from sr_gan_fd_amd.gan import GanTrainer
    nodes, mean, std = ["features.2", "features.7", "features.16", "features.25", "features.34"], [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    A.set_dry_run(True)
    gc.collect()
    gc.disable()
    try:
        for dfac in (lambda: M.discriminator_unet(in_channels=3, out_channels=1, channels=64), M.uNetDiscriminatorAesrgan, M.discriminator):
            g, d, cl, cl1 = M.bsrgan_x4(num_rrdb=1), dfac(), M.ContentLoss(nodes, mean, std), M.ContentLoss("features.34", mean, std)
            if dfac is M.discriminator:
                x = torch.rand(2, 3, 128, 128, requires_grad=True)
                d(x).sum().backward()
                sr = torch.rand(2, 3, 32, 32, requires_grad=True)
                cl1(sr, torch.rand(2, 3, 32, 32)).backward()
                y = g(torch.rand(2, 3, 16, 16))
                y.sum().backward()
                del x, sr, y
            else:
                tr = GanTrainer(g, d, cl)
                tr.step(torch.rand(2, 3, 16, 16), torch.rand(2, 3, 64, 64))
                del tr
            del g, d, cl, cl1
            gc.set_debug(gc.DEBUG_SAVEALL)
            gc.collect()
            leaked = []
            for o in gc.garbage:
                name = type(o).__name__            # (type(), not isinstance(): dead weakref proxies sit in the garbage list too)
                if type(o) is torch.Tensor or "Engine" in name or name in ("_Shape", "FlatParams"):
                    leaked.append(name)
            gc.garbage.clear()
            gc.set_debug(0)
            assert not leaked, f"kept alive only by reference cycles: {sorted(set(leaked))} ({len(leaked)} objects)"
    finally:
        gc.set_debug(0)
        gc.garbage.clear()
        gc.enable()
        A.set_dry_run(False)


def test_fused_optimizer_checkpoint_round_trip(tmp_path):
    """FlatAdamEMA.state_dict() / load_state_dict() speak torch.optim.Adam's per-parameter format and AveragedModel's
    ``module.<name>`` + ``n_averaged`` layout (the reference's checkpoint, train_bsrnet.py:124-130): a state written by
    torch's own classes loads into the flat buffers and comes back identical."""
    from torch.optim.swa_utils import AveragedModel
    from sr_gan_fd_amd import model as M, utils
    from sr_gan_fd_amd.engine import FlatParams
    from sr_gan_fd_amd.trainer import FlatAdamEMA
    torch.manual_seed(0)
    net = M.bsrgan_x4(num_rrdb=1)
    opt = torch.optim.Adam(net.parameters(), 1e-4, (0.9, 0.99), 1e-4, 0.0)
    ema = AveragedModel(net, avg_fn=lambda a, p, n: 0.001 * a + 0.999 * p)
    for _ in range(3):
        for p in net.parameters():
            p.grad = torch.randn_like(p) * 1e-3
        opt.step()
        ema.update_parameters(net)
    path = str(tmp_path / "g_last.pth.tar")
    torch.save({"epoch": 7, "best_psnr": 1.0, "best_ssim": 2.0, "state_dict": net.state_dict(), "ema_state_dict": ema.state_dict(),
                "optimizer": opt.state_dict()}, path)

    net2 = M.bsrgan_x4(num_rrdb=1)
    fp = FlatParams(list(net2.named_parameters()))
    flat = fp.sync(torch.device("cpu"))
    fused = FlatAdamEMA(flat, 5e-5, (0.9, 0.999), 1e-8, 0.0, ema_decay=0.999, layout=fp)
    out = utils.load_state_dict(net2, path, ema_model=fused, optimizer=fused, load_mode="resume")
    assert out[2] == 7 and fused.t == 3 and fused.n_averaged == 3 and fused.lr == 1e-4 and fused.eps == 1e-4 and fused.betas == (0.9, 0.99)
    for (k, a), b in zip(net.state_dict().items(), net2.state_dict().values()):
        assert torch.equal(a, b), k
    want = opt.state_dict()["state"]
    got = fused.state_dict()
    assert got["param_groups"][0]["params"] == list(range(len(want)))
    for i in want:
        assert torch.equal(want[i]["exp_avg"], got["state"][i]["exp_avg"]) and torch.equal(want[i]["exp_avg_sq"], got["state"][i]["exp_avg_sq"])
        assert float(got["state"][i]["step"]) == 3.0
    for k, v in ema.state_dict().items():
        assert torch.equal(v, fused.ema_state_dict()[k]), k
    # and back into torch's own classes (what the reference's resume path does with a file the fused trainer wrote)
    utils.save_checkpoint(str(tmp_path / "again.pth.tar"), net2, fused, ema=fused, epoch=8)
    net3 = M.bsrgan_x4(num_rrdb=1)
    opt3 = torch.optim.Adam(net3.parameters(), 1.0)
    ema3 = AveragedModel(net3)
    utils.load_state_dict(net3, str(tmp_path / "again.pth.tar"), ema_model=ema3, optimizer=opt3, load_mode="resume")
    assert opt3.state_dict()["param_groups"][0]["lr"] == 1e-4
    for i in want:
        assert torch.equal(opt3.state_dict()["state"][i]["exp_avg_sq"], want[i]["exp_avg_sq"])
    assert int(ema3.n_averaged) == 3


def test_plan_cache_keeps_training_plan():
    from sr_gan_fd_amd.engine import PlanCache
    c = PlanCache(cap=3, cap_pinned=2)
    c.put("train", "T", pinned=True)
    for i in range(10):
        c.put(("eval", i), i)
    assert c.get("train") == "T" and len(c) == 4 and c.get(("eval", 9)) == 9 and c.get(("eval", 0)) is None
    c.put("train2", "T2", pinned=True); c.put("train3", "T3", pinned=True)
    assert c.get("train") is None and c.get("train3") == "T3"


def test_multistep_lr_mirror_follows_torch_and_exchanges_state():
    """trainer.MultiStepLR == torch.optim.lr_scheduler.MultiStepLR (bsrgan_config.py:153-155 milestones / gamma, one step per
    epoch: train_bsrgan.py:193-195) on the fused optimizer, and the two load each other's state_dict (checkpoint key "scheduler")."""
    from sr_gan_fd_amd.trainer import FlatAdamEMA, MultiStepLR
    flat = torch.zeros(8)
    fused = FlatAdamEMA(flat, 8e-5, (0.9, 0.999), 1e-4)
    ref_p = torch.nn.Parameter(torch.zeros(8))
    ref_opt = torch.optim.Adam([ref_p], 8e-5)
    milestones, gamma = [2, 5, 5, 9], 0.5          # a repeated milestone applies gamma twice (torch keeps a Counter)
    mine, ref = MultiStepLR(fused, milestones, gamma), torch.optim.lr_scheduler.MultiStepLR(ref_opt, milestones, gamma)
    for epoch in range(12):
        assert abs(fused.lr - ref_opt.param_groups[0]["lr"]) < 1e-18 and mine.get_last_lr() == ref.get_last_lr(), epoch
        if epoch == 6:
            # resume in the middle: each implementation continues from the other's state
            fused2 = FlatAdamEMA(torch.zeros(8), 1.0, (0.9, 0.999), 1e-4)
            mine2 = MultiStepLR(fused2, [1], 0.1)
            mine2.load_state_dict(ref.state_dict())
            ref_opt2 = torch.optim.Adam([torch.nn.Parameter(torch.zeros(8))], 1.0)
            ref2 = torch.optim.lr_scheduler.MultiStepLR(ref_opt2, [1], 0.1)
            ref2.load_state_dict(mine.state_dict())
            ref_opt2.param_groups[0]["lr"] = ref2.get_last_lr()[0]      # torch restores the rate with the optimizer's own state
            assert fused2.lr == fused.lr and mine2.last_epoch == ref.last_epoch
        ref_opt.step()
        mine.step()
        ref.step()
        if epoch >= 6:
            ref_opt2.step()
            mine2.step()
            ref2.step()
            assert abs(fused2.lr - fused.lr) < 1e-18 and abs(ref_opt2.param_groups[0]["lr"] - fused.lr) < 1e-18, epoch


# ------------------------------------------------------------------------------------------------
# Input shape contracts (dry run): every entry point refuses a wrong shape on the host, before a plan is built or anything launches.
# On a GPU each refused call below would be an out-of-bounds read (a boundary kernel or a loss kernel sized by the other operand).
# ------------------------------------------------------------------------------------------------
_NODES5 = ["features.2", "features.7", "features.16", "features.25", "features.34"]
_MEAN, _STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def _unet():
    from sr_gan_fd_amd import model as M
    return M.discriminator_unet(in_channels=3, out_channels=1, channels=64)


def _engines_of(*modules):
    from sr_gan_fd_amd import engine as E
    return [E._ENGINES[m] for m in modules if m in E._ENGINES]


def _nothing_planned(*modules):
    """no engine of these modules has built a plan or run a forward (shape checks come first)"""
    return all(len(e.shapes) == 0 and e.token == 0 for e in _engines_of(*modules))


def _refused_calls():
    """(id, call) pairs: each call must raise SrganfdError before anything is planned; the modules it touches are returned by the call
    through the list it is given, so the test can check that nothing was planned for them"""
    from sr_gan_fd_amd import model as M
    from sr_gan_fd_amd.gan import GanTrainer
    from sr_gan_fd_amd.gan_esrgan import EsrganGanTrainer
    from sr_gan_fd_amd.trainer import GeneratorTrainer
    r = torch.rand

    def g_trainer_gt_too_small(mods):
        g = M.bsrgan_x4(num_rrdb=1)
        mods += [g]
        GeneratorTrainer(g, lr=1e-4).step(r(2, 3, 16, 16), r(2, 3, 32, 32))           # sr would be 2x3x64x64

    def gan_trainer_gt_too_small(mods):
        g, d = M.bsrgan_x4(num_rrdb=1), M.uNetDiscriminatorAesrgan()
        mods += [g, d]
        GanTrainer(g, d).step(r(2, 3, 16, 16), r(2, 3, 32, 32))

    def gan_trainer_generator_first_gt_usm_wrong(mods):
        g, d = M.RRDBNet(num_rrdb=1, upscale_factor=2), _unet()
        mods += [g, d]
        GanTrainer(g, d, generator_first=True).step(r(2, 3, 16, 16), r(2, 3, 32, 32), r(2, 3, 64, 64))

    def gan_trainer_generator_first_gt_wrong(mods):
        g, d = M.RRDBNet(num_rrdb=1, upscale_factor=1), _unet()
        mods += [g, d]
        GanTrainer(g, d, generator_first=True).step(r(2, 3, 16, 16), r(2, 3, 64, 64), r(2, 3, 16, 16))

    def esrgan_trainer_x2_gt_of_x4(mods):
        g, d = M.RRDBNet(num_rrdb=1, upscale_factor=2), M.discriminator()
        mods += [g, d]
        EsrganGanTrainer(g, d).step(r(2, 3, 32, 32), r(2, 3, 128, 128))             # x2 from 32: sr is 64x64

    def generator_four_channel_image(mods):
        g = M.bsrgan_x4(num_rrdb=1)
        mods += [g]
        g(r(2, 4, 16, 16))

    def generator_x2_channels_after_unshuffle(mods):
        g = M.RRDBNet(num_rrdb=1, upscale_factor=2)
        mods += [g]
        g(r(2, 12, 8, 8))                                                          # an already unshuffled input is not an image

    def generator_x1_size_not_divisible(mods):
        g = M.RRDBNet(num_rrdb=1, upscale_factor=1)
        mods += [g]
        g(r(2, 3, 16, 18))                                                         # PixelUnshuffle(4) needs multiples of 4

    def generator_trainer_x2_odd_size(mods):
        g = M.RRDBNet(num_rrdb=1, upscale_factor=2)
        mods += [g]
        GeneratorTrainer(g, lr=1e-4).step(r(2, 3, 15, 16), r(2, 3, 30, 32))

    def generator_not_4d(mods):
        g = M.bsrgan_x4(num_rrdb=1)
        mods += [g]
        g(r(3, 16, 16))

    def unet_one_channel(mods):
        d = _unet()
        mods += [d]
        d(r(2, 1, 32, 32))

    def aesrgan_d_one_channel(mods):
        d = M.uNetDiscriminatorAesrgan()
        mods += [d]
        d(r(2, 1, 32, 32))

    def esrgan_d_one_channel(mods):
        d = M.discriminator()
        mods += [d]
        d(r(2, 1, 128, 128))

    def esrgan_d_64(mods):
        d = M.discriminator()
        mods += [d]
        d(r(2, 3, 64, 64))

    def rrdb_block_half_channels(mods):
        blk = M.BSRGAN(num_rrdb=1).trunk[0]
        mods += [blk]
        blk(r(1, 32, 16, 16))                                                      # a 64-channel block

    def rdb_block_not_4d(mods):
        blk = M.BSRGAN(num_rrdb=1).trunk[0].rdb1
        mods += [blk]
        blk(r(64, 16, 16))
    return [(f.__name__, f) for f in (g_trainer_gt_too_small, gan_trainer_gt_too_small, gan_trainer_generator_first_gt_usm_wrong,
                                      gan_trainer_generator_first_gt_wrong, esrgan_trainer_x2_gt_of_x4, generator_four_channel_image,
                                      generator_x2_channels_after_unshuffle, generator_x1_size_not_divisible, generator_trainer_x2_odd_size,
                                      generator_not_4d, unet_one_channel, aesrgan_d_one_channel, esrgan_d_one_channel, esrgan_d_64,
                                      rrdb_block_half_channels, rdb_block_not_4d)]


@pytest.mark.parametrize("name", [n for n, _ in _refused_calls()])
def test_wrong_shapes_are_refused_before_any_launch(name):
    """Each of these returned normally before the shape contracts existed (and on a GPU read past the end of an input or target
    buffer), except the ESRGAN discriminator at 64x64, which was refused only after its weights were packed.  Now each raises
    SrganfdError naming the shape it got, and no engine involved has built a plan or run a forward."""
    from sr_gan_fd_amd import _abi as A
    call = dict(_refused_calls())[name]
    A.set_dry_run(True)
    try:
        mods = []
        with pytest.raises(A.SrganfdError, match=r"got shape|has shape"):
            call(mods)
        assert _nothing_planned(*mods), name
    finally:
        A.set_dry_run(False)


@pytest.mark.parametrize("s", [2, 1])
def test_real_esrgan_below_x4_fused_trainers_produce_the_gt_shape(s):
    """Real-ESRGAN's RRDBNet at x2 / x1 (Real_ESRGAN/model.py:190-204,248): the fused trainers go through the same PixelUnshuffle as the
    module path, so SR has the GT's shape and the dense blocks run at 1 / unshuffle of the LR size.  (The trainers used to hand the
    3-channel image to a conv1 that reads 12 / 48 channels and return a 4x-sized SR.)"""
    from sr_gan_fd_amd import _abi as A, model as M
    from sr_gan_fd_amd.gan import GanTrainer
    from sr_gan_fd_amd.gan_esrgan import EsrganGanTrainer
    from sr_gan_fd_amd.trainer import GeneratorTrainer
    u = 4 // s
    A.set_dry_run(True)
    try:
        lr, gt = torch.rand(2, 3, 16, 24), torch.rand(2, 3, 16 * s, 24 * s)
        tr = GeneratorTrainer(M.RRDBNet(num_rrdb=1, upscale_factor=s), lr=1e-4)
        tr.step(lr, gt)
        assert tr.sr.shape == gt.shape
        assert (tr.eng._last.H, tr.eng._last.W) == (16 // u, 24 // u)
        for order in (False, True):
            tr = GanTrainer(M.RRDBNet(num_rrdb=1, upscale_factor=s), _unet(), M.ContentLoss(_NODES5, _MEAN, _STD), generator_first=order)
            assert tr.step(lr, gt, gt.clone() if order else None).shape == (8,)
            assert tr.sr.shape == gt.shape and tr.content_vals.shape == (1, 5)
        lr_e = torch.rand(2, 3, 128 // s, 128 // s)                 # the ESRGAN discriminator takes 128x128 only
        tr = EsrganGanTrainer(M.RRDBNet(num_rrdb=1, upscale_factor=s), M.discriminator(), M.ContentLoss("features.34", _MEAN, _STD))
        assert tr.step(lr_e, torch.rand(2, 3, 128, 128)).shape == (8,)
        assert tr.sr.shape == (2, 3, 128, 128)
    finally:
        A.set_dry_run(False)


@pytest.mark.parametrize("s", [2, 1])
def test_real_esrgan_below_x4_module_forward_unshuffles_once(s):
    """The module path still returns 4 / unshuffle times the input size, with the unshuffle applied once (by the engine): the plan
    is built at the trunk's size, and the training and inference forwards agree on shapes."""
    from sr_gan_fd_amd import _abi as A, engine as E, model as M
    u = 4 // s
    A.set_dry_run(True)
    try:
        net = M.RRDBNet(num_rrdb=1, upscale_factor=s)
        net.compute_dtype = torch.float32
        x = torch.rand(2, 3, 16, 24)
        sr = net(x)
        assert sr.shape == (2, 3, 16 * s, 24 * s)
        eng = E.generator_engine(net)
        assert (eng._last.N, eng._last.H, eng._last.W) == (2, 16 // u, 24 // u)
        assert eng.output_shape(x.shape) == tuple(sr.shape)
        sr.sum().backward()
        assert net.conv1.weight.grad.shape == (64, 3 * u * u, 3, 3)
        with torch.no_grad():
            assert net(x).shape == sr.shape
    finally:
        A.set_dry_run(False)
