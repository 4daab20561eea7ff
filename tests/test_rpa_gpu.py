"""srganfd_pixel_gate and the modules RPA, US and Generator_RPA on the GPU (sr_gan_fd_amd/csrc/pixel_gate.hip, engine_rpa.py) against
float64: the formula at op level, the torch-CPU restatement (tests/rpa_oracle.py, pinned to the reference by tests/golden/rpa.npz)
for the modules.  The cases (rpa_oracle.CASES) are the smallest at which the launches can go wrong -- odd sizes, more than one
image, one and two US blocks, none -- and were chosen under the conditions tests/test_rpa_host.py checks (a gate that is not
degenerate, no LeakyReLU pre-activation near zero, caps on E).

Op level   largest absolute difference over the tensor's largest magnitude in float64.  f32: 8 float32 epsilons.  f16 / bf16: one
           rounding of the stored type (its unit roundoff) plus the same 8 epsilons.  |a| reaches 20 and 90: the sigmoid's tails
           neither overflow nor give NaN.  Outputs sit inside allocations filled with 0xFF bytes (NaN in all three types): every
           byte outside the written slice stays 0xFF and no NaN is left inside.  Two runs give the same bits; da over dz in place
           gives the bits of the out-of-place run.
Modules    per tensor -- out, dx and every parameter gradient.
  f32      largest absolute difference over the tensor's largest magnitude in the float64 oracle; bound 8 G, G the oracle's own
           float32-vs-float64 gap, computed live (the factor: tests/test_attention_gpu.py, tests/test_lpips_gpu.py).
  f16, bf16  relative L2 error; bound max(2 E, 8 G), E the gap of the oracle with that type's rounding points, G as above, both
           computed live in the same norm; E <= 0.05 for f16 and <= 0.15 for bf16.  L2 and not the maximum, because a stored 16-bit
           pre-activation that rounds across zero moves a whole receptive field; the same rounding points keep that rare, not
           impossible.  With bf16's bound up to 0.3 the bf16 run only catches whole-tensor mistakes: the f32 and f16 runs are what
           catch a single wrong row.
  A bias gradient that is a plain sum of the incoming gradient (the generator's conv3.bias: eighths) has E = G = 0: equality.
  test_matches_oracle prints every error / bound ratio.  Largest ratio per case on the MI355X: f32 0.19-0.47, f16 0.50-0.67, bf16
  0.50-0.51 (0.5 = an error equal to E); op level f32 0.19, f16 0.72, bf16 0.91.  DESIGN.md 4e has the table.
Exact      a second forward + backward and the forward without a graph (whose plan shares activation buffers among the blocks) give
           the same bits; the images of a batch run one by one give the batch's out and dx bits; a US block's output equals, bit for
           bit, conv2 launched over an explicitly up-sampled copy of the low-resolution gate output.
"""
import pytest
import torch

from tests import rpa_oracle as RO

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
EPS32 = 2.0 ** -23
GUARD = 4096                                    # bytes on either side, a multiple of the 16-byte alignment the kernel asks for


# ---- op level ----
def banded(npix, cstride, tdt):
    """(raw bytes incl. guards, the (npix, cstride) tensor inside), everything 0xFF"""
    nbytes = npix * cstride * torch.empty(0, dtype=tdt).element_size()
    raw = torch.full((nbytes + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    return raw, raw[GUARD:GUARD + nbytes].view(tdt).view(npix, cstride)


def check_written(raw, inner, c0, c, what):
    """nothing outside channels [c0, c0 + c) of ``inner`` was written, and every element inside was"""
    assert bool((raw[:GUARD] == 0xFF).all()) and bool((raw[-GUARD:] == 0xFF).all()), what + ": bytes outside the tensor were written"
    es = inner.element_size()
    by = inner.view(torch.uint8).view(inner.shape[0], inner.shape[1] * es)
    outside = torch.ones(inner.shape[1] * es, dtype=torch.bool, device=DEV)
    outside[c0 * es:(c0 + c) * es] = False
    assert bool((by[:, outside] == 0xFF).all()), what + ": channels outside the slice were written"
    assert not bool(torch.isnan(inner[:, c0:c0 + c].float()).any()), what + ": NaN (or an element never written) inside"


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("sliced", [False, True], ids=["dense", "sliced"])
@pytest.mark.parametrize("npix", [35, 2 * 19 * 23])
@pytest.mark.parametrize("c", [32, 64])
def test_pixel_gate_op(c, npix, sliced, dt):
    from sr_gan_fd_amd import _abi as A, ops
    tdt = DTYPES[dt]
    dtc = ops.DT[tdt]
    cstride, c0 = (96, 32) if sliced else (c, 0)
    g = torch.Generator().manual_seed(11 + c + npix)
    x = torch.randn(npix, c, generator=g).to(tdt)
    a = (torch.randn(npix, c, generator=g) * 4).to(tdt)
    a[:, 0], a[:, 1], a[0, 2], a[0, 3] = 20.0, -20.0, 90.0, -90.0
    dz = torch.randn(npix, c, generator=g).to(tdt)
    x64, a64, dz64 = x.double(), a.double(), dz.double()
    s = torch.sigmoid(a64)
    want = {"z": x64 * (1 + s), "dx": dz64 * (1 + s), "da": dz64 * x64 * s * (1 - s)}

    def place(t):
        buf = torch.zeros(npix, cstride, dtype=tdt)
        buf[:, c0:c0 + c] = t
        return buf.to(DEV)
    bx, ba, bdz = place(x), place(a), place(dz)
    V = lambda t: A.view(t, c0=c0)

    def run(in_place):
        out = {k: banded(npix, cstride, tdt) for k in ("z", "dx", "da")}
        if in_place:
            out["da"][1][:, c0:c0 + c] = bdz[:, c0:c0 + c]
        ops.pixel_gate(ops.pixel_gate_args(dtc, npix, c, V(bx), V(ba), z=V(out["z"][1])))
        ops.pixel_gate(ops.pixel_gate_args(dtc, npix, c, V(bx), V(ba), dz=V(out["da"][1]) if in_place else V(bdz), dx=V(out["dx"][1]), da=V(out["da"][1])))
        torch.cuda.synchronize()
        return out
    first, second, third = run(False), run(False), run(True)
    bound = 8 * EPS32 + (0.0 if dt == "f32" else torch.finfo(tdt).eps / 2)
    for k, ref in want.items():
        raw, inner = first[k]
        check_written(raw, inner, c0, c, k)
        check_written(*third[k], c0, c, k + " (in place)")
        got = inner[:, c0:c0 + c].cpu()
        assert bool(torch.isfinite(got.float()).all()), k
        err = float((got.double() - ref).abs().max() / ref.abs().max())
        print("pixel_gate %-4s c %d npix %d %-6s %-2s err %.3e bound %.3e ratio %.3f" % (dt, c, npix, "sliced" if sliced else "dense", k, err, bound, err / bound))
        assert err <= bound, (k, err, bound)
        assert torch.equal(first[k][0], second[k][0]), "two runs differ in " + k
        assert torch.equal(first[k][0], third[k][0]), "da written in place over dz changes " + k


# ---- modules ----
def module(name, dt):
    from sr_gan_fd_amd import model as M
    kind, _, nf, nb, scale, _ = RO.CASES[name]
    m = {"rpa": lambda: M.RPA(nf), "us": lambda: M.US(nf, 2), "gen": lambda: M.Generator_RPA(scale=scale, num_feat=nf, num_block=nb)}[kind]()
    m.load_state_dict(RO.runs(name)["state"])
    m.compute_dtype = dt
    return m.to(DEV)


def run(m, x, d_out):
    """forward + backward of the module: out, dx and every parameter gradient, on the CPU"""
    m.zero_grad(set_to_none=True)
    xg = x.to(DEV).requires_grad_(True)
    out = m(xg)
    out.backward(d_out.to(DEV))
    torch.cuda.synchronize()
    res = {"out": out.detach().cpu(), "dx": xg.grad.cpu()}
    for k, p in m.named_parameters():
        res[k] = p.grad.detach().cpu().clone()
    return res


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", list(RO.CASES))
def test_matches_oracle(name, dt):
    r = RO.runs(name)
    got = run(module(name, DTYPES[dt]), r["x"], r["d_out"])
    ref = r["f64"]
    assert set(got) == set(ref)
    bad, worst = [], 0.0
    for k in ref:
        assert got[k].shape == ref[k].shape and got[k].dtype == torch.float32, k
        if dt == "f32":
            err, bound, what = RO.max_gap(got[k], ref[k]), 8 * RO.max_gap(r["f32"][k], ref[k]), "8G"
        else:
            E, G = RO.l2_gap(r[dt][k], ref[k]), RO.l2_gap(r["f32"][k], ref[k])
            assert E <= (0.05 if dt == "f16" else 0.15), (k, E)
            err, bound, what = RO.l2_gap(got[k], ref[k]), max(2 * E, 8 * G), "max(2E, 8G)"
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))      # a bias gradient that sums eighths: exact in every precision
        worst = max(worst, ratio)
        print("%-10s %-4s %-28s err %.3e  %s %.3e  ratio %.3f" % (name, dt, k, err, what, bound, ratio))
        if not err <= bound:
            bad.append((k, err, bound))
    print("%-10s %-4s largest ratio %.3f" % (name, dt, worst))
    assert not bad, bad


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", ["rpa_5x7", "us_5x7", "gen2_5x7", "gen4_4x6"])
def test_exactness(name, dt):
    r = RO.runs(name)
    m = module(name, DTYPES[dt])
    a = run(m, r["x"], r["d_out"])
    b = run(m, r["x"], r["d_out"])
    for k in a:
        assert torch.equal(a[k], b[k]), "two runs differ in " + k
    with torch.no_grad():                       # the inference plan shares activation buffers among the blocks: the same launches, the same bits
        assert torch.equal(m(r["x"].to(DEV)).cpu(), a["out"]), "the forward without a graph differs"
    if r["x"].shape[0] == 2:
        for i in range(2):
            one = run(m, r["x"][i:i + 1], r["d_out"][i:i + 1])
            for k in ("out", "dx"):
                assert torch.equal(a[k][i:i + 1], one[k]), "image %d alone differs in %s" % (i, k)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_us_rewrite_is_exact(dt):
    """the per-pixel layers run before the up-sampling: conv2 through its fused nearest-x2 read gives the bits of conv2 over an
    explicitly up-sampled copy of the low-resolution gate output"""
    from sr_gan_fd_amd import _abi as A, ops
    from sr_gan_fd_amd.engine_rpa import rpa_engine
    r = RO.runs("us_5x7")
    m = module("us_5x7", DTYPES[dt])
    with torch.no_grad():
        out = m(r["x"].to(DEV))
    eng = rpa_engine(m, "us")
    sp, dtc = eng._last, ops.DT[DTYPES[dt]]
    rec = sp.recs[0]
    n, h, w, f = rec.g.shape
    g_up = rec.g.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).contiguous()
    assert g_up.shape == (n, 2 * h, 2 * w, f)
    y = torch.empty_like(rec.y)
    pk = eng.packed[dtc]
    bias = eng.fp.flat.data_ptr() + 4 * eng.fp.off("conv2.bias")
    ops.conv2d(ops.conv_args(dtc, A.view(g_up), A.view(y), pk["buf"].data_ptr() + pk["offs"][("f", "conv2")], n, 2 * h, 2 * w, f, f, bias=bias,
                             act=A.ACT_LRELU, slope=0.2))
    torch.cuda.synchronize()
    assert torch.equal(y, rec.y)
    assert torch.equal(out, y.float().permute(0, 3, 1, 2))


# ---- protocol ----
def test_autocast_picks_the_dtype():
    from sr_gan_fd_amd import _abi as A
    from sr_gan_fd_amd.engine_rpa import rpa_engine
    r = RO.runs("gen2_9x6")
    m = module("gen2_9x6", None)
    x = r["x"].to(DEV)
    with torch.autocast("cuda"):
        out = m(x)
        assert rpa_engine(m, "gen")._last.dtc == A.F16 and out.dtype == torch.float32
        out.backward(r["d_out"].to(DEV))
    grads = [p.grad for p in m.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grads)
    m.zero_grad(set_to_none=True)
    out = m(x)
    assert rpa_engine(m, "gen")._last.dtc == A.F32
    assert RO.max_gap(out.detach().cpu(), r["f64"]["out"]) <= 8 * RO.max_gap(r["f32"]["out"], r["f64"]["out"])
    with torch.autocast("cuda", dtype=torch.bfloat16):
        m(x)
        assert rpa_engine(m, "gen")._last.dtc == A.BF16


@pytest.mark.parametrize("name", ["rpa_5x7", "gen2_9x6"])
def test_frozen_parameters_get_no_gradient(name):
    r = RO.runs(name)
    m = module(name, torch.float32)
    full = run(m, r["x"], r["d_out"])
    for p in m.parameters():
        p.requires_grad_(False)
    m.zero_grad(set_to_none=True)
    xg = r["x"].to(DEV).requires_grad_(True)
    m(xg).backward(r["d_out"].to(DEV))
    assert all(p.grad is None for p in m.parameters())
    assert torch.equal(xg.grad.cpu(), full["dx"])
    assert RO.max_gap(xg.grad.cpu(), r["f64"]["dx"]) <= 8 * RO.max_gap(r["f32"]["dx"], r["f64"]["dx"])


def test_second_forward_before_backward_raises():
    from sr_gan_fd_amd import _abi as A
    r = RO.runs("rpa_5x7")
    m = module("rpa_5x7", torch.float16)
    first = m(r["x"].to(DEV))
    m(r["x"].to(DEV))
    with pytest.raises(A.SrganfdError, match="overwritten by a later forward"):
        first.backward(r["d_out"].to(DEV))


def test_factory_constructs_and_runs(capsys):
    from sr_gan_fd_amd import model as M
    capsys.readouterr()
    g = M.__dict__["gen_rpa2x"]()
    assert capsys.readouterr().out == "* Generator_RPA 2x\n"
    with torch.no_grad():
        out = g.to(DEV)(torch.rand(1, 3, 8, 8, device=DEV))
    torch.cuda.synchronize()
    assert out.shape == (1, 3, 16, 16) and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
