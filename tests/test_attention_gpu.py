"""SelfAttention on the GPU (sr_gan_fd_amd/csrc/attention.hip, attention.py, model.SelfAttention) against the torch-CPU
restatement run in float64 (tests/attention_oracle.py), on the five cases of attention_oracle.CASES: the smallest shapes at which
the tiling can go wrong (a ragged last key tile, D = 16 / 32 / 64, a sequence shorter than any tile, several query blocks, exact
tile multiples).  Inputs follow attention_oracle.make_case: a peaked softmax, under which a mis-indexed key or head moves a result
by the order of its magnitude.

Every error is the largest absolute difference over a tensor, relative to the tensor's largest magnitude in the float64 oracle.
Compared: the output, the head-averaged weights, d x and the four parameter gradients.

  f32 mode   bound 8 G per tensor.  G is that tensor's gap between the float32 and the float64 run of the same oracle, computed
             live on the CPU; the factor 8 is the project's precedent for another accumulation order (tests/test_lpips_gpu.py).
             G on an x86-64 host over the six shapes: out 1.0-1.9e-6, weights 0.5-2.2e-6, dx 2.1-2.9e-6, in_proj_weight 0.7-2.4e-6,
             in_proj_bias 0.6-2.1e-6, out_proj.weight 0.8-1.8e-6; out_proj.bias 0 (see below).
  f16, bf16  bound 2 E per tensor, E being the gap between the oracle with that type's rounding points and the plain float64 oracle
             (the kernels round at the same points and differ in accumulation order, which can flip single roundings but not change
             the error's scale), and E <= 0.05 so that the bound stays far below an indexing error.  E on an x86-64 host: f16
             0.6-2.1e-3, bf16 1.0-3.3e-2 over the tensors and shapes -- except out_proj.bias, whose gradient is the plain sum of the
             incoming gradient and does not depend on the forward at all: E = 0 exactly.  A 16-bit bound is never taken below the
             f32 mode's own, max(2 E, 8 G): the 16-bit paths accumulate in fp32 like the f32 one.  For every other tensor 2 E is a
             hundred times 8 G and the bound is the 2 E as stated.  The incoming gradient is drawn in eighths (attention_oracle.
             make_case), which every type here holds and sums exactly, so for out_proj.bias G is 0 too and the check is equality.
  MI355X     largest error / bound over the six shapes: f32 0.20-0.30 per tensor; f16 0.50-0.77, bf16 0.50-0.60 (0.5 = an error
             equal to E); out_proj.bias exact.
  exact      rows of the weights sum to 1 within 1e-6; need_weights = False, a second run, and the images of a batch run one by
             one all give the same bits (no atomics; every output element has one owner and a fixed summation order).
  guard bands (op level)  out, lse, weights and d_qkv sit inside larger allocations filled with 0xFF bytes (NaN in all three
             types): every byte outside stays 0xFF and no NaN is left inside, so every element was written and nothing else.

test_matches_oracle prints every error / bound ratio; DESIGN.md 4d has the table."""
import functools

import pytest
import torch

from tests import attention_oracle as AO

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
KEYS = ("out", "weights", "dx") + AO.PARAMS
IDS = ["%s%d" % c for c in AO.CASE_IDS]


@functools.lru_cache(maxsize=None)
def oracle(name, i):
    """inputs and the four oracle runs of one case, computed once and shared"""
    c, heads, x, state, d_out = AO.case_inputs(name, i)
    runs = {"f64": AO.self_attention(x, state, heads, d_out=d_out),
            "f32": AO.self_attention(x, state, heads, dtype=torch.float32, d_out=d_out),
            "f16": AO.self_attention(x, state, heads, emulate=torch.float16, d_out=d_out),
            "bf16": AO.self_attention(x, state, heads, emulate=torch.bfloat16, d_out=d_out)}
    return c, heads, x, state, d_out, runs


def gap(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


def module(c, heads, state, dt):
    from sr_gan_fd_amd import model as M
    m = M.SelfAttention(c, heads)
    m.load_state_dict(state)
    m.compute_dtype = dt
    return m.to(DEV)


def run(m, x, d_out):
    """forward + backward of the module: the seven tensors on the CPU"""
    m.zero_grad(set_to_none=True)
    xg = x.to(DEV).requires_grad_(True)
    out, weights = m(xg)
    out.backward(d_out.to(DEV))
    torch.cuda.synchronize()
    res = {"out": out.detach().cpu(), "weights": None if weights is None else weights.cpu(), "dx": xg.grad.cpu()}
    for k in AO.PARAMS:
        res[k] = m.multihead_attention.get_parameter(k).grad.detach().cpu().clone()
    return res


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("case", AO.CASE_IDS, ids=IDS)
def test_matches_oracle(case, dt):
    c, heads, x, state, d_out, runs = oracle(*case)
    got = run(module(c, heads, state, DTYPES[dt]), x, d_out)
    ref = runs["f64"]
    bad = []
    for k in KEYS:
        assert got[k].shape == ref[k].shape and got[k].dtype == torch.float32, k
        err, G = gap(got[k], ref[k]), gap(runs["f32"][k], ref[k])
        if dt == "f32":
            bound, what = 8 * G, "8G"
        else:
            E = gap(runs[dt][k], ref[k])
            assert E <= 0.05, (k, E)
            bound, what = max(2 * E, 8 * G), "max(2E, 8G)"
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))      # out_proj.bias: sums of eighths, exact in every precision
        print("%s%d %-4s %-16s err %.3e  %s %.3e  ratio %.3f" % (case + (dt, k, err, what, bound, ratio)))
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, bad


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("case", AO.CASE_IDS, ids=IDS)
def test_exactness(case, dt):
    c, heads, x, state, d_out, _ = oracle(*case)
    m = module(c, heads, state, DTYPES[dt])
    a = run(m, x, d_out)
    assert (a["weights"].double().sum(-1) - 1).abs().max() <= 1e-6
    b = run(m, x, d_out)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), "two runs differ in " + k
    m.need_weights = False
    n = run(m, x, d_out)
    assert n["weights"] is None
    for k in KEYS:
        if k != "weights":
            assert torch.equal(a[k], n[k]), "need_weights=False changes " + k
    m.need_weights = True
    if x.shape[0] == 2:
        for i in range(2):
            one = run(m, x[i:i + 1], d_out[i:i + 1])
            for k in ("out", "weights", "dx"):
                assert torch.equal(a[k][i:i + 1], one[k]), "image %d alone differs in %s" % (i, k)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("case", [("A", 0), ("D", 0)], ids=["A0", "D0"])
def test_guard_bands(case, dt):
    from sr_gan_fd_amd import ops
    c, heads, shapes = AO.CASES[case[0]]
    b, h, w = shapes[case[1]]
    L, D, tdt = h * w, c // heads, DTYPES[dt]
    dtc, es = ops.DT[tdt], ops.esize(ops.DT[tdt])
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(b, L, 3 * c, generator=g).to(tdt).to(DEV)
    d_out = torch.randn(b, L, c, generator=g).to(tdt).to(DEV)
    GUARD = 4096                                    # bytes on either side, a multiple of the 16-byte alignment the kernels ask for

    def banded(numel, dtype):
        nbytes = numel * torch.empty(0, dtype=dtype).element_size()
        raw = torch.full((nbytes + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        return raw, raw[GUARD:GUARD + nbytes].view(dtype)
    bufs = {"out": banded(b * L * c, tdt), "lse": banded(b * heads * L, torch.float32), "weights": banded(b * L * L, torch.float32),
            "d_qkv": banded(b * L * 3 * c, tdt)}
    t = {k: v[1] for k, v in bufs.items()}
    ops.attention_fwd(ops.attn_args(dtc, b, L, heads, D, qkv=qkv, out=t["out"], lse=t["lse"]))
    ops.attention_weights(ops.attn_args(dtc, b, L, heads, D, qkv=qkv, lse=t["lse"], weights=t["weights"]))
    need = ops.attention_workspace_bytes(ops.attn_args(dtc, b, L, heads, D))
    assert need == 4 * b * heads * L
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    ops.attention_bwd(ops.attn_args(dtc, b, L, heads, D, qkv=qkv, out=t["out"], lse=t["lse"], d_out=d_out, d_qkv=t["d_qkv"], workspace=ws))
    torch.cuda.synchronize()
    assert es * t["out"].numel() == bufs["out"][0].numel() - 2 * GUARD
    for k, (raw, inner) in bufs.items():
        assert bool((raw[:GUARD] == 0xFF).all()) and bool((raw[-GUARD:] == 0xFF).all()), k + ": bytes outside the tensor were written"
        assert not bool(torch.isnan(inner.float()).any()), k + ": NaN (or an element never written) inside"


def test_autocast_picks_the_dtype_and_fills_the_gradients():
    from sr_gan_fd_amd import _abi as A
    from sr_gan_fd_amd.attention import attention_engine
    c, heads, x, state, _, runs = oracle("A", 0)
    m = module(c, heads, state, None)
    with torch.autocast("cuda"):
        out, _ = m(x.to(DEV))
        assert attention_engine(m)._last.dtc == A.F16 and out.dtype == torch.float32
        out.sum().backward()
    grads = [p.grad for p in m.parameters()]
    assert len(grads) == 4 and all(g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grads)
    m.zero_grad(set_to_none=True)
    out, _ = m(x.to(DEV))
    assert attention_engine(m)._last.dtc == A.F32
    assert gap(out.detach().cpu(), runs["f64"]["out"]) <= 8 * gap(runs["f32"]["out"], runs["f64"]["out"])
    with torch.autocast("cuda", dtype=torch.bfloat16):
        m(x.to(DEV))
        assert attention_engine(m)._last.dtc == A.BF16


def test_graph_capture_replays_the_eager_step():
    """forward + backward of the bare module captured once by graph.GraphedStep (any object with ``step(a, b)`` fits it) and
    replayed on other data: the same bits as the eager run"""
    from sr_gan_fd_amd.graph import GraphedStep
    c, heads, x, state, d_out, _ = oracle("A", 0)
    m = module(c, heads, state, torch.float16)

    class Step:
        pg = None

        def __init__(self):
            self.x = None

        def step(self, xs, ds):
            m.zero_grad(set_to_none=True)
            self.x = xs.detach().requires_grad_(True)
            out, weights = m(self.x)
            out.backward(ds)
            return [out.detach(), weights, self.x.grad] + [p.grad for p in m.parameters()]
    eager = [t.clone() for t in Step().step(x.to(DEV), d_out.to(DEV))]
    graphed = GraphedStep(Step(), torch.zeros_like(x, device=DEV), torch.ones_like(d_out, device=DEV), warmup=1)
    got = graphed(x.to(DEV), d_out.to(DEV))
    torch.cuda.synchronize()
    assert len(got) == len(eager) == 7
    for i, (a, b) in enumerate(zip(eager, got)):
        assert torch.equal(a, b), "tensor %d of the replay differs from the eager step" % i
