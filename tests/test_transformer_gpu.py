"""TransformerEncoderLayer / TransformerEncoder on the GPU (sr_gan_fd_amd/transformer.py, csrc/layernorm.hip, csrc/attention_seq.hip
and the 1x1 launches of the conv and weight-gradient kernels) against the torch-CPU restatement run in float64
(tests/transformer_oracle.py), on the five cases of transformer_oracle.CASES -- the smallest shapes at which the launches can go
wrong -- in f32, f16 and bf16.  tests/test_transformer_host.py checks, on the oracle alone, that the cases are well conditioned.

Op level   add_layernorm forward and backward and dropout_apply against the float64 formula over the same inputs; the largest
           absolute difference over the tensor's largest magnitude in float64.  f32: 8 float32 epsilons.  f16 / bf16: one rounding of
           the stored type (its unit roundoff) plus the same 8 epsilons (tests/test_rpa_gpu.py's op-level bounds).  LayerNorm
           normalises the z it STORED, so y, mean and rstd are held against the formula over that z, and the backward against the
           formula over the forward's z, mean and rstd.  Token counts 35 and 2 * 19 * 23, E 64 and 128, with and without a keep-mask.
           Outputs sit in 0xFF-filled guard bands (NaN in all three types): nothing outside is written, no NaN is left inside; two
           runs give the same bits.  The short-sequence attention's outputs sit in guard bands too.
Modules    out, d src and every parameter gradient against the oracle in relative L2, in eval mode and in train mode with p = 0.1,
           the oracle replaying the module's own ``dropout_masks()``.  f32: 8 G; f16 / bf16: max(2 E, 8 G), with G the oracle's own
           float32-vs-float64 gap and E its gap with that type's rounding points, both computed live for the same masks.
           test_matches_oracle prints every error / bound ratio.
           MI355X, error / bound over the five cases and all tensors: eval f32 0.10-0.24, f16 0.46-0.54, bf16 0.48-0.52; train f32
           0.11-0.22, f16 0.45-0.61, bf16 0.47-0.57 (0.5 = an error equal to E); the last layer's norm2.bias, the plain sum of a gradient
           drawn in eighths, is exact.  Op level: add_layernorm f32 <= 0.17, f16 <= 0.85, bf16 <= 0.95; dropout_apply <= 0.09 / 0.69 /
           0.69.  DESIGN.md 4g has the table per case.
Exact      two forward + backward passes give the same bits; train mode with p = 0 gives eval's bits; a one-layer TransformerEncoder
           gives the lone layer's bits; a graph-captured eval step replays the eager bits.
Orientation  permuting the images along S permutes the output rows the same way (attention without positions is equivariant, and
           every other piece is per token); one sequence alone (an N = 1 slice) gives that column's bits."""
import functools

import pytest
import torch

from tests import transformer_oracle as TO

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
EPS32 = float(torch.finfo(torch.float32).eps)
GUARD = 4096                                            # bytes on either side, a multiple of the 16-byte alignment the kernels ask for


def banded(shape, dtype):
    """a tensor of ``shape`` inside a larger allocation filled with 0xFF bytes: (raw bytes, the tensor)"""
    numel = 1
    for s in shape:
        numel *= s
    nbytes = numel * torch.empty(0, dtype=dtype).element_size()
    raw = torch.full((nbytes + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    return raw, raw[GUARD:GUARD + nbytes].view(dtype).view(*shape)


def check_written(raw, inner, what):
    assert bool((raw[:GUARD] == 0xFF).all()) and bool((raw[-GUARD:] == 0xFF).all()), what + ": bytes outside the tensor were written"
    assert not bool(torch.isnan(inner.float()).any()), what + ": NaN (or an element never written) inside"


def op_bound(dt):
    return 8 * EPS32 + (0.0 if dt == "f32" else float(torch.finfo(DTYPES[dt]).eps) / 2)


def rel_max(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


# ---- op level ----
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "keep"])
@pytest.mark.parametrize("ntok", [35, 2 * 19 * 23])
@pytest.mark.parametrize("e", [64, 128])
def test_add_layernorm_op(e, ntok, masked, dt):
    from sr_gan_fd_amd import ops
    tdt, dtc, bound = DTYPES[dt], ops.DT[DTYPES[dt]], op_bound(dt)
    g = torch.Generator().manual_seed(13 + e + ntok)
    x, r, dy = (torch.randn(ntok, e, generator=g).to(tdt) for _ in range(3))
    gamma, beta = 1.0 + 0.2 * torch.randn(e, generator=g), 0.2 * torch.randn(e, generator=g)
    keep = (torch.rand(ntok, e, generator=g) >= 0.25).to(torch.uint8) if masked else None
    scale, eps = (1.0 / 0.75 if masked else 1.0), 1e-5
    f64 = 1.0 if keep is None else keep.double() * scale
    dev = lambda t: None if t is None else t.to(DEV)
    dx_, dr_, dy_, keep_, gamma_, beta_ = dev(x), dev(r), dev(dy), dev(keep), dev(gamma), dev(beta)
    ws = torch.empty(ops.add_layernorm_workspace_bytes(ntok, e), dtype=torch.uint8, device=DEV)

    def run():
        o = {"z": banded((ntok, e), tdt), "y": banded((ntok, e), tdt), "mean": banded((ntok,), torch.float32), "rstd": banded((ntok,), torch.float32),
             "dx": banded((ntok, e), tdt), "dr": banded((ntok, e), tdt), "grad": banded((2 * e,), torch.float32)}
        t = {k: v[1] for k, v in o.items()}
        ops.launch_alone(ops.AddLayerNorm(dtc, ntok, e, x=dx_, r=dr_, keep=keep_, keep_scale=scale, gamma=gamma_.data_ptr(), beta=beta_.data_ptr(), eps=eps,
                                          z=t["z"], y=t["y"], mean=t["mean"], rstd=t["rstd"]))
        item = ops.AddLayerNorm(dtc, ntok, e, dy=dy_, z=t["z"], mean=t["mean"], rstd=t["rstd"], gamma=gamma_.data_ptr(), keep=keep_, keep_scale=scale,
                                dx=t["dx"], dr=t["dr"], dg_off=0, db_off=e, ws=ws)
        run_ = ops.Run(item.kind, grad=t["grad"].data_ptr())
        item.launch(run_)
        torch.cuda.synchronize()
        return o
    first, second = run(), run()
    for k, (raw, inner) in first.items():
        check_written(raw, inner, k)
        assert torch.equal(raw, second[k][0]), "two runs differ in " + k
    got = {k: v[1].cpu() for k, v in first.items()}
    z = got["z"].double()                                            # LayerNorm normalises what it stored
    mu = z.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((z - mu) ** 2).mean(-1, keepdim=True) + eps)
    want = {"z": x.double() + r.double() * f64, "mean": mu[:, 0], "rstd": rstd[:, 0], "y": (z - mu) * rstd * gamma.double() + beta.double()}
    # the backward over the forward's own z, mean and rstd
    xh = (z - got["mean"].double()[:, None]) * got["rstd"].double()[:, None]
    gg = dy.double() * gamma.double()
    dz = got["rstd"].double()[:, None] * (gg - gg.mean(-1, keepdim=True) - xh * (gg * xh).mean(-1, keepdim=True))
    want.update(dx=dz, dr=dz * f64, grad=torch.cat([(dy.double() * xh).sum(0), dy.double().sum(0)]))
    for k, ref in want.items():
        b = bound if k in ("z", "y", "dx", "dr") else 8 * EPS32      # mean, rstd and the parameter gradients are fp32 in every mode
        err = rel_max(got[k], ref)
        print("add_layernorm %-4s e %d ntok %d %-5s %-4s err %.3e bound %.3e ratio %.3f" % (dt, e, ntok, "keep" if masked else "plain", k, err, b, err / b))
        assert err <= b, (k, err, b)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("numel", [35 * 64, 2 * 19 * 23 * 128])
def test_dropout_apply_op(numel, dt):
    from sr_gan_fd_amd import ops
    tdt, dtc = DTYPES[dt], ops.DT[DTYPES[dt]]
    g = torch.Generator().manual_seed(17 + numel)
    x = torch.randn(numel, generator=g).to(tdt)
    keep = (torch.rand(numel, generator=g) >= 0.1).to(torch.uint8)
    want = x.double() * keep.double() / 0.9
    x_, keep_ = x.to(DEV), keep.to(DEV)

    def run(in_place):
        raw, y = banded((numel,), tdt)
        if in_place:
            y.copy_(x_)
        ops.launch_alone(ops.DropoutApply(dtc, y if in_place else x_, keep_, 1.0 / 0.9, y, numel))
        torch.cuda.synchronize()
        return raw, y
    first, second, third = run(False), run(False), run(True)
    check_written(*first, "y")
    assert torch.equal(first[0], second[0]) and torch.equal(first[0], third[0]), "a second run, or the run in place, gives other bits"
    err, bound = rel_max(first[1], want), op_bound(dt)
    print("dropout_apply %-4s numel %d err %.3e bound %.3e ratio %.3f" % (dt, numel, err, bound, err / bound))
    assert err <= bound
    assert bool((first[1].cpu()[keep == 0] == 0).all())


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("shape", [(3, 35, 4, 16), (5, 35, 4, 32), (8, 9, 2, 64)], ids=["D16", "D32", "D64"])
def test_seq_attention_guard_bands(shape, dt):
    from sr_gan_fd_amd import ops
    S, N, H, D = shape
    C, tdt = H * D, DTYPES[dt]
    dtc = ops.DT[tdt]
    g = torch.Generator().manual_seed(19)
    qkv = torch.randn(S, N, 3 * C, generator=g).to(tdt).to(DEV)
    d_out = torch.randn(S, N, C, generator=g).to(tdt).to(DEV)
    keep = (torch.rand(N, H, S, S, generator=g) >= 0.1).to(torch.uint8).to(DEV)
    bufs = {"out": banded((S, N, C), tdt), "lse": banded((N, H, S), torch.float32), "d_qkv": banded((S, N, 3 * C), tdt)}
    t = {k: v[1] for k, v in bufs.items()}
    aa = lambda **kw: ops.seq_attn_args(dtc, S, N, H, D, qkv=qkv, out=t["out"], lse=t["lse"], keep=keep, keep_scale=1.0 / 0.9, **kw)
    ops.launch_alone(ops.SeqAttention("fwd", aa()))
    ops.launch_alone(ops.SeqAttention("bwd", aa(d_out=d_out, d_qkv=t["d_qkv"])))
    torch.cuda.synchronize()
    for k, (raw, inner) in bufs.items():
        check_written(raw, inner, k)


# ---- modules ----
def module(name, dt, train=False, p=TO.P_TRAIN, lone=False):
    from sr_gan_fd_amd import model as M
    S, N, E, heads, F, layers = TO.CASES[name]
    layer = M.TransformerEncoderLayer(E, heads, F, p)
    m = layer if lone else M.TransformerEncoder(layer, layers)
    state = TO.eval_runs(name)["state"]
    m.load_state_dict({k[len("layers.0."):]: v for k, v in state.items()} if lone else state)
    m.compute_dtype = dt
    return m.to(DEV).train(train)


def run(m, src, d_out):
    """forward + backward of the module: out, dsrc and every parameter gradient, on the CPU"""
    m.zero_grad(set_to_none=True)
    xg = src.to(DEV).requires_grad_(True)
    out = m(xg)
    out.backward(d_out.to(DEV))
    torch.cuda.synchronize()
    res = {"out": out.detach().cpu(), "dsrc": xg.grad.cpu()}
    for k, p in m.named_parameters():
        res[k] = p.grad.detach().cpu().clone()
    return res


@functools.lru_cache(maxsize=None)
def train_runs(name, dt):
    """a train-mode step of the module (seeded) and the oracle's four runs over the module's own masks"""
    r = TO.eval_runs(name)
    m = module(name, DTYPES[dt], train=True)
    torch.manual_seed(4)
    got = run(m, r["src"], r["d_out"])
    masks = {k: v.cpu() for k, v in m.dropout_masks().items()}
    S, N, E, heads, F, layers = TO.CASES[name]
    assert sorted(masks) == sorted("layers.%d.%s" % (i, s) for i in range(layers) for s in TO.SITES)
    for k, t in masks.items():
        assert t.dtype == torch.uint8 and int(t.max()) <= 1 and 0.0 < float(t.float().mean()) < 1.0, k + ": not a mixed 0 / 1 mask"
    return got, TO.all_runs(r["src"], r["state"], heads, r["d_out"], masks, TO.P_TRAIN)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("name", list(TO.CASES))
def test_matches_oracle(name, mode, dt):
    if mode == "eval":
        runs = TO.eval_runs(name)
        got = run(module(name, DTYPES[dt]), runs["src"], runs["d_out"])
    else:
        got, runs = train_runs(name, dt)
    ref, bad = runs["f64"], []
    assert set(got) == set(ref)
    for k in ref:
        assert got[k].shape == ref[k].shape and got[k].dtype == torch.float32, k
        err, G = TO.rel_l2(got[k], ref[k]), TO.rel_l2(runs["f32"][k], ref[k])
        if dt == "f32":
            bound, what = 8 * G, "8G"
        else:
            E = TO.rel_l2(runs[dt][k], ref[k])
            assert E <= (0.05 if dt == "f16" else 0.15), (k, E)
            bound, what = max(2 * E, 8 * G), "max(2E, 8G)"
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        print("%-10s %-5s %-4s %-36s err %.3e  %s %.3e  ratio %.3f" % (name, mode, dt, k, err, what, bound, ratio))
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, bad


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", ["odd_seq", "two_layers"])
def test_exactness(name, dt):
    r = TO.eval_runs(name)
    m = module(name, DTYPES[dt])
    a, b = run(m, r["src"], r["d_out"]), run(m, r["src"], r["d_out"])
    for k in a:
        assert torch.equal(a[k], b[k]), "two runs differ in " + k
    c = run(module(name, DTYPES[dt], train=True, p=0.0), r["src"], r["d_out"])            # train mode, p = 0: no masks, eval's bits
    for k in a:
        assert torch.equal(a[k], c[k]), "train mode with p = 0 differs from eval mode in " + k
    m.train()                                                                             # p = 0.1: seeded masks, two runs agree
    torch.manual_seed(8)
    d = run(m, r["src"], r["d_out"])
    torch.manual_seed(8)
    e = run(m, r["src"], r["d_out"])
    assert not torch.equal(a["out"], d["out"])
    for k in d:
        assert torch.equal(d[k], e[k]), "two seeded train-mode runs differ in " + k
    f = run(m, r["src"], r["d_out"])                                                      # not re-seeded: other masks
    assert not torch.equal(d["out"], f["out"])


@pytest.mark.parametrize("dt", list(DTYPES))
def test_one_layer_stack_is_the_lone_layer(dt):
    r = TO.eval_runs("odd_seq")
    a = run(module("odd_seq", DTYPES[dt]), r["src"], r["d_out"])
    b = run(module("odd_seq", DTYPES[dt], lone=True), r["src"], r["d_out"])
    assert set(a) == {"out", "dsrc"} | {"layers.0." + k for k in TO.LAYER_PARAMS}
    for k in a:
        assert torch.equal(a[k], b[k[len("layers.0."):] if k.startswith("layers.0.") else k]), k


@pytest.mark.parametrize("dt", list(DTYPES))
def test_orientation(dt):
    r = TO.eval_runs("two_layers")
    m = module("two_layers", DTYPES[dt])
    src, d_out = r["src"], r["d_out"]
    a = run(m, src, d_out)
    perm = torch.tensor([3, 0, 7, 1, 6, 2, 5, 4])
    b = run(m, src[perm].contiguous(), d_out[perm].contiguous())
    # every token attends over the same keys in another order, so the sums differ in their last bits.  The float64 oracle is
    # equivariant exactly and each run lies within the module-level bound of it: twice that bound holds between the two runs
    for k in ("out", "dsrc"):
        G = TO.rel_l2(r["f32"][k], r["f64"][k])
        bound = 2 * (8 * G if dt == "f32" else max(2 * TO.rel_l2(r[dt][k], r["f64"][k]), 8 * G))
        assert TO.rel_l2(b[k], a[k][perm]) <= bound, (k, bound)
    assert TO.rel_l2(b["out"], a["out"]) > 0.1                        # ... and it is the S axis that carries the sequence
    for n in (0, 77, 129):                                            # one sequence alone: that column's bits
        one = run(m, src[:, n:n + 1].contiguous(), d_out[:, n:n + 1].contiguous())
        for k in ("out", "dsrc"):
            assert torch.equal(one[k], a[k][:, n:n + 1]), "sequence %d alone differs in %s" % (n, k)


def test_autocast_picks_the_dtype():
    from sr_gan_fd_amd import _abi as A
    from sr_gan_fd_amd.transformer import transformer_engine
    r = TO.eval_runs("odd_seq")
    m = module("odd_seq", None)
    with torch.autocast("cuda"):
        out = m(r["src"].to(DEV))
        assert transformer_engine(m)._last.dtc == A.F16 and out.dtype == torch.float32
        out.sum().backward()
    grads = [p.grad for p in m.parameters()]
    assert len(grads) == 12 and all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    m(r["src"].to(DEV))
    assert transformer_engine(m)._last.dtc == A.F32
    with torch.autocast("cuda", dtype=torch.bfloat16):
        m(r["src"].to(DEV))
        assert transformer_engine(m)._last.dtc == A.BF16


def test_graph_capture_replays_the_eager_step():
    """forward + backward of the eval-mode stack captured once by graph.GraphedStep and replayed on other data: the eager bits"""
    from sr_gan_fd_amd.graph import GraphedStep
    r = TO.eval_runs("two_layers")
    m = module("two_layers", torch.float16)
    src, d_out = r["src"], r["d_out"]

    class Step:
        pg = None

        def step(self, xs, ds):
            m.zero_grad(set_to_none=True)
            x = xs.detach().requires_grad_(True)
            out = m(x)
            out.backward(ds)
            return [out.detach(), x.grad] + [p.grad for p in m.parameters()]
    eager = [t.clone() for t in Step().step(src.to(DEV), d_out.to(DEV))]
    graphed = GraphedStep(Step(), torch.zeros_like(src, device=DEV), torch.ones_like(d_out, device=DEV), warmup=1)
    got = graphed(src.to(DEV), d_out.to(DEV))
    torch.cuda.synchronize()
    assert len(got) == len(eager) == 26
    for i, (a, b) in enumerate(zip(eager, got)):
        assert torch.equal(a, b), "tensor %d of the replay differs from the eager step" % i
