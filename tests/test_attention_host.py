"""Host-side checks of SelfAttention (no GPU: the library runs in dry-run mode, where every entry point validates its arguments and
launches nothing): the float64 oracle against the reference's own outputs (tests/golden/attention.npz, written by
tests/golden/make_golden_attention.py), the input recipe's peakedness, the module's parameters, every SRGANFD_EINVAL path of the
four entry points, and the sequence of calls a forward + backward of the module makes."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import attention_oracle as AO

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention.npz")


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


def test_fixture_is_small_and_on_the_float16_grid(golden):
    assert os.path.getsize(FIXTURE) < 1 << 20
    for k, v in golden.items():
        assert v.dtype == (np.float64 if k.endswith((".out", ".weights")) else np.float16), k


@pytest.mark.parametrize("name", ["A", "C"])
def test_oracle_reproduces_the_reference(golden, name):
    c, heads, x, state, _ = AO.case_inputs(name)
    assert np.array_equal(golden[name + ".x"].astype(np.float32), x.numpy())                       # the recipe still gives the fixture's inputs
    for k, v in state.items():
        assert np.array_equal(golden[name + ".state." + k].astype(np.float32), v.numpy()), k
    res = AO.self_attention(x, state, heads)
    for k in ("out", "weights"):
        want = torch.from_numpy(golden[name + "." + k])
        assert res[k].shape == want.shape
        assert float((res[k] - want).abs().max() / want.abs().max()) <= 1e-12, k


@pytest.mark.parametrize("case", AO.CASE_IDS, ids=["%s%d" % c for c in AO.CASE_IDS])
def test_recipe_gives_a_peaked_softmax(case):
    c, heads, x, state, _ = AO.case_inputs(*case)
    weights = AO.self_attention(x, state, heads)["weights"]
    assert float((weights.sum(-1) - 1).abs().max()) < 1e-12
    assert AO.peakedness(weights) >= 3.0                   # mean row maximum >= 3 / L


def test_parameters_are_multihead_attentions():
    from sr_gan_fd_amd import model as M
    torch.manual_seed(3)
    m = M.SelfAttention(64, 4)
    torch.manual_seed(3)
    want = torch.nn.MultiheadAttention(64, 4).state_dict()
    got = m.state_dict()
    assert list(got) == ["multihead_attention." + k for k in want]
    assert list(got) == [AO.PREFIX + k for k in AO.PARAMS]
    for k, v in want.items():
        assert torch.equal(got["multihead_attention." + k], v), k
    assert (m.channels, m.num_heads, m.need_weights, m.compute_dtype) == (64, 4, True, None)
    assert M.SelfAttention(256).num_heads == 8
    assert isinstance(m.multihead_attention, torch.nn.MultiheadAttention)


def test_bsrgansa_has_bsrgans_keys():
    from sr_gan_fd_amd import model as M
    torch.manual_seed(0)
    a = M.bsrgansa_x2(num_rrdb=1)
    torch.manual_seed(0)
    b = M.bsrgan_x2(num_rrdb=1)
    assert isinstance(a, M.BSRGANsa) and a.upscale_factor == 2
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert M.__dict__["bsrgansa_x2"] is M.bsrgansa_x2 and "SelfAttention" in M.__all__


def test_abi_version_stays_7():
    from sr_gan_fd_amd import _abi as A
    assert A.lib().srganfd_abi_version() == A.ABI_VERSION == 7
    for name in ("srganfd_attention_fwd", "srganfd_attention_weights", "srganfd_attention_bwd", "srganfd_attention_workspace_bytes"):
        assert name in A.SYMBOLS and hasattr(A.lib(), name)


def _buffers(b=2, L=36, heads=8, D=32):
    c = heads * D
    return dict(qkv=torch.zeros(b, L, 3 * c), out=torch.zeros(b, L, c), lse=torch.zeros(b, heads, L), d_out=torch.zeros(b, L, c),
                d_qkv=torch.zeros(b, L, 3 * c), weights=torch.zeros(b, L, L), workspace=torch.zeros(b * heads * L))


USES = {"fwd": ("qkv", "out", "lse"), "weights": ("qkv", "lse", "weights"), "bwd": ("qkv", "out", "lse", "d_out", "d_qkv", "workspace")}


def _call(A, entry, args):
    rc = getattr(A.lib(), "srganfd_attention_" + entry)(C.byref(args), None)
    return rc, A.lib().srganfd_last_error().decode()


def test_entry_points_refuse_bad_arguments(dry_run):
    from sr_gan_fd_amd import ops
    A = dry_run
    EINVAL = -1
    t = _buffers()
    good = lambda **kw: ops.attn_args(A.F32, 2, 36, 8, 32, **{**t, **kw})
    for entry, uses in USES.items():
        assert _call(A, entry, good())[0] == 0, entry
        for name in uses:                                             # a null pointer among those the entry point uses
            rc, msg = _call(A, entry, good(**{name: None}))
            assert rc == EINVAL and "null pointer" in msg and entry in msg, (entry, name, msg)
        for field, value, text in (("head_dim", 8, "head_dim 8"), ("head_dim", 128, "head_dim 128"), ("batch", 0, "non-positive"),
                                   ("seq", 0, "non-positive"), ("heads", -1, "non-positive"), ("dtype", 5, "bad dtype")):
            a = good()
            setattr(a, field, value)
            rc, msg = _call(A, entry, a)
            assert rc == EINVAL and text in msg and entry in msg, (entry, field, msg)
        rc, msg = _call(A, entry, good(qkv=t["qkv"].view(-1)[1:]))     # 4 bytes off a 16-byte boundary
        assert rc == EINVAL and "aligned" in msg, (entry, msg)
    assert A.lib().srganfd_attention_fwd(None, None) == EINVAL and "null arguments" in A.lib().srganfd_last_error().decode()
    rc, msg = _call(A, "fwd", good(out=t["qkv"]))
    assert rc == EINVAL and "aliases" in msg
    rc, msg = _call(A, "bwd", good(d_qkv=t["qkv"]))
    assert rc == EINVAL and "d_qkv aliases qkv" in msg
    rc, msg = _call(A, "bwd", good(workspace=t["workspace"][:-1]))
    assert rc == EINVAL and "workspace too small" in msg
    # the query: bytes for delta (batch, heads, seq) fp32; 0 and an error text for arguments no kernel takes
    assert ops.attention_workspace_bytes(ops.attn_args(A.F16, 2, 36, 8, 32)) == 2 * 8 * 36 * 4
    bad = ops.attn_args(A.F16, 2, 36, 8, 48)
    assert A.lib().srganfd_attention_workspace_bytes(C.byref(bad)) == 0 and "head_dim 48" in A.lib().srganfd_last_error().decode()
    with pytest.raises(A.SrganfdError, match="head_dim 48"):
        ops.attention_workspace_bytes(bad)


class _Calls:
    """stands in for the library handle: notes the name of every call that enqueues work, then makes it"""
    QUIET = ("srganfd_last_error", "srganfd_set_dry_run", "srganfd_abi_version", "srganfd_pack_layout", "srganfd_wgrad_plan_bytes",
             "srganfd_wgrad_plan_build", "srganfd_pack_weights")

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


FORWARD = ["nchw_to_nhwc", "conv2d", "attention_fwd", "attention_weights", "conv2d", "nhwc_to_nchw"]
BACKWARD = ["nchw_to_nhwc", "conv2d_wgrad", "conv2d", "attention_bwd", "conv2d_wgrad", "conv2d", "nhwc_to_nchw"]


@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.bfloat16])
def test_module_call_sequence(dry_run, dt):
    from sr_gan_fd_amd import model as M
    A = dry_run
    m = M.SelfAttention(256, 8)
    m.compute_dtype = dt
    rec = _Calls(A.lib())
    A._lib = rec
    try:
        x = torch.randn(2, 256, 6, 6, requires_grad=True)
        out, weights = m(x)
        assert out.shape == (2, 256, 6, 6) and weights.shape == (2, 36, 36) and not weights.requires_grad
        assert rec.names == FORWARD
        out.sum().backward()
        assert rec.names == FORWARD + BACKWARD
        assert x.grad.shape == x.shape and all(p.grad is not None and p.grad.shape == p.shape for p in m.parameters())
        del rec.names[:]
        m.need_weights = False                                  # no weights launch, None in their place
        out, weights = m(x)
        assert weights is None and rec.names == [n for n in FORWARD if n != "attention_weights"]
        del rec.names[:]
        for p in m.parameters():                                # frozen parameters: no weight-gradient launches
            p.requires_grad_(False)
        m(x)[0].sum().backward()
        assert rec.names == [n for n in FORWARD if n != "attention_weights"] + [n for n in BACKWARD if n != "conv2d_wgrad"]
        del rec.names[:]
        with torch.no_grad():                                   # no graph: the forward alone
            m(x.detach())
        assert rec.names == [n for n in FORWARD if n != "attention_weights"]
    finally:
        A._lib = rec._lib


def test_module_refuses_what_has_no_kernel(dry_run):
    from sr_gan_fd_amd import model as M
    A = dry_run
    with pytest.raises(A.SrganfdError, match="not a multiple of num_heads"):
        M.SelfAttention(100, 8)
    with pytest.raises(A.SrganfdError, match="head size 8"):
        M.SelfAttention(64, 8)(torch.randn(1, 64, 4, 4))
    with pytest.raises(A.SrganfdError, match=r"expects \(N, 64, H, W\)"):
        M.SelfAttention(64, 4)(torch.randn(1, 32, 4, 4))
    A.set_dry_run(False)
    with pytest.raises(A.SrganfdError, match="not on a GPU"):
        M.SelfAttention(64, 4)(torch.randn(1, 64, 4, 4))


def test_compute_dtype_pins_the_precision(dry_run):
    """fp32 outside autocast, ``compute_dtype`` as the override (the autocast side needs a GPU: tests/test_attention_gpu.py)"""
    from sr_gan_fd_amd import model as M
    from sr_gan_fd_amd.attention import attention_engine
    A = dry_run
    m = M.SelfAttention(64, 4)
    x = torch.randn(3, 64, 2, 4)
    m(x)
    assert attention_engine(m)._last.dtc == A.F32
    for dt, code in ((torch.float16, A.F16), (torch.bfloat16, A.BF16)):
        m.compute_dtype = dt
        m(x)
        assert attention_engine(m)._last.dtc == code
    m.compute_dtype = torch.float64
    with pytest.raises(A.SrganfdError, match="not supported"):
        m(x)
