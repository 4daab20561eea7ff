"""tests/thin_oracle.py is itself checked (no GPU): the three formulas against torch's own float64 conv2d / conv_transpose2d and against
autograd -- and the case tables of tests/test_thin_paths_gpu.py against the dispatch of csrc/conv_thin.hip: the launches they build,
asked for their kernel label with dummy pointers (srganfd_conv2d_thin_describe launches nothing), must reach every labelled
instantiation of the three kernel templates and no other."""
import pytest
import torch
import torch.nn.functional as F

from tests import thin_oracle as T
from tests import test_thin_paths_gpu as P

F64 = torch.float64


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _operands(cs, seed):
    torch.manual_seed(seed)
    n, h, w = 2, 6, 9
    thin = torch.zeros(n, h, w, 4, dtype=F64)
    thin[..., :cs] = torch.randn(n, h, w, cs, dtype=F64)
    return thin, torch.randn(n, h, w, 64, dtype=F64), torch.randn(n, h, w, 64, dtype=F64)


@pytest.mark.parametrize("cs", P.CS)
def test_thin_in_is_conv2d_and_the_masked_data_gradient(cs):
    thin, _, mask = _operands(cs, cs)
    x = _nchw(thin[..., :cs])
    w, b = torch.randn(64, cs, 3, 3, dtype=F64), torch.randn(64, dtype=F64)
    y, A = T.thin_in(thin, w, cs, w_big_is_cout=True, bias=b, act=T.ACT_LRELU, slope=0.2)
    assert torch.allclose(y, _nhwc(F.leaky_relu(F.conv2d(x, w, b, padding=1), 0.2)), rtol=1e-12, atol=1e-12)
    assert bool((A >= y.abs() * (1 - 1e-12)).all())
    y, _ = T.thin_in(thin, w, cs, w_big_is_cout=True, bias=b, act=T.ACT_RELU)
    assert torch.allclose(y, _nhwc(F.relu(F.conv2d(x, w, b, padding=1))), rtol=1e-12, atol=1e-12)
    # the data gradient of a 64 -> cs conv with weight wo: conv_transpose2d of dy (the thin side), times LeakyReLU'(mask)
    wo = torch.randn(cs, 64, 3, 3, dtype=F64)
    y, _ = T.thin_in(thin, wo, cs, w_big_is_cout=False, flip=True, mask=mask, mask_slope=0.3)
    factor = torch.where(mask > 0, torch.ones_like(mask), torch.full_like(mask, 0.3))
    assert torch.allclose(y, _nhwc(F.conv_transpose2d(x, wo, padding=1)) * factor, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("cs", P.CS)
def test_thin_out_is_conv2d_and_the_data_gradient(cs):
    _, big, _ = _operands(cs, 10 + cs)
    wo, b = torch.randn(cs, 64, 3, 3, dtype=F64), torch.randn(cs, dtype=F64)
    y, A = T.thin_out(big, wo, cs, w_big_is_cout=False, bias=b)
    assert torch.allclose(y, _nhwc(F.conv2d(_nchw(big), wo, b, padding=1)), rtol=1e-12, atol=1e-12) and bool((A >= y.abs() * (1 - 1e-12)).all())
    wi = torch.randn(64, cs, 3, 3, dtype=F64)
    y, _ = T.thin_out(big, wi, cs, w_big_is_cout=True, flip=True)
    assert torch.allclose(y, _nhwc(F.conv_transpose2d(_nchw(big), wi, padding=1)), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("cs", P.CS)
@pytest.mark.parametrize("big_is_cout", [True, False])
def test_thin_wgrad_is_autograd(cs, big_is_cout):
    thin, big, _ = _operands(cs, 20 + cs)
    small = _nchw(thin[..., :cs])
    if big_is_cout:          # conv: thin (cs) -> big (64); x = thin, dy = big
        wp, bp = torch.zeros(64, cs, 3, 3, dtype=F64, requires_grad=True), torch.zeros(64, dtype=F64, requires_grad=True)
        (F.conv2d(small, wp, bp, padding=1) * _nchw(big)).sum().backward()
    else:                    # conv: big (64) -> thin (cs); x = big, dy = thin
        wp, bp = torch.zeros(cs, 64, 3, 3, dtype=F64, requires_grad=True), torch.zeros(cs, dtype=F64, requires_grad=True)
        (F.conv2d(_nchw(big), wp, bp, padding=1) * small).sum().backward()
    dw, db, A_dw, A_db = T.thin_wgrad(big, thin, cs, w_big_is_cout=big_is_cout)
    assert dw.shape == wp.shape and torch.allclose(dw, wp.grad, rtol=1e-12, atol=1e-12)
    assert db.shape == bp.shape and torch.allclose(db, bp.grad, rtol=1e-12, atol=1e-12)
    assert bool((A_dw >= dw.abs() * (1 - 1e-12)).all()) and bool((A_db >= db.abs() * (1 - 1e-12)).all())


def test_masked_bound_is_two_roundings():
    ref, A = torch.tensor([1.0, -3.0], dtype=F64), torch.tensor([2.0, 5.0], dtype=F64)
    for dt in P.HALF:
        extra = T.bound_in(ref, A, 3, dt, True) - T.bound_in(ref, A, 3, dt, False)
        assert torch.equal(extra, T.O.ROUND_U[dt] * ref.abs())


# the 12 labelled instantiations of csrc/conv_thin.hip (the thirteenth kernel, the slab reduction, follows every thin_wgrad launch)
INSTANTIATIONS = ({f"thin_in_kernel<{t}{m}{nt}>" for t in ("bf16", "f16") for m in ("", ",mask") for nt in ("", ",NT")}
                  | {f"thin_{k}_kernel<{t}>" for k in ("out", "wgrad") for t in ("bf16", "f16")})


def test_cases_reach_every_instantiation_and_no_other():
    from sr_gan_fd_amd import _abi as A, ops
    assert len(INSTANTIATIONS) == 12
    A.set_dry_run(True)
    try:
        seen = set()
        for a, op, lab in P.dummy_launches():
            got = ops.thin_describe(a, op)
            assert got == lab, (got, lab)
            seen.add(got)
        assert seen == INSTANTIATIONS, (sorted(INSTANTIATIONS - seen), sorted(seen - INSTANTIATIONS))
        # the several-units case: the grid comes from the workspace query (256 compute units in dry-run mode)
        ws = ops.thin_wgrad_workspace_bytes()
        assert ws == 2 * 256 * P.SLAB_BYTES
        n, h, w = P.wgrad_units_shape(ws)
        waves = 8 * (ws // P.SLAB_BYTES)
        assert (n, h, w) == (8, 520, 33) and 2 * waves < n * h * 2 < 3 * waves
        with pytest.raises(A.SrganfdError, match="op 3"):
            ops.thin_describe(a, 3)
    finally:
        A.set_dry_run(False)


def test_case_tables_cover_what_they_promise():
    assert P.SHAPES[:5] == [(2, 16, 16), (1, 37, 52), (2, 33, 70), (1, 64, 129), (3, 5, 7)] and P.SHAPES[5] == (1, 1, 1)
    assert {cs for _, cs in P.IN_CASES} == {cs for _, cs in P.OUT_CASES if _ != "fwd_bias_pitch1_slice"} == {cs for _, cs, _ in P.WG_CASES} == {1, 2, 3, 4}
    masks = {P.IN_MODES[m][4] for m, _ in P.IN_CASES}
    assert masks == {None, P.DENSE, P.PLANAR192, P.SLICE96}
    assert {P.IN_MODES[m][5] for m, _ in P.IN_CASES} == {P.DENSE, P.SLICE96, P.PLANAR192}
    assert {(P.OUT_MODES[m][3], cs) for m, cs in P.OUT_CASES} >= {(1, 1), (4, 1), (4, 4)} and any(P.OUT_MODES[m][4][1] for m, _ in P.OUT_CASES)
    assert {(P.WG_MODES[m][0][2], bool(P.WG_MODES[m][0][1]), P.WG_MODES[m][1]) for m, _, _ in P.WG_CASES} >= {(0, False, True), (0, True, False), (1, True, True), (1, True, False)}
    n, h, w = P.NT_SHAPE
    assert [n * h * w * c * 2 >= P.NT_BYTES for _, c, _ in P.NT_CASES] == [nt for _, _, nt in P.NT_CASES] == [True, True, False]
