"""Host-side checks of tests/esrgan_d_oracle.py, the float64 checker of ESRGAN's BatchNorm discriminator and of the differentiable VGG
content loss (no GPU):

  * the oracle IS the reference's network: in float32, without rounding points or replayed states, it reproduces what the reference's own
    Discriminator computed (tests/golden/esrgan_discriminator.npz) within the f32 bounds tests/test_esrgan_d_gpu.py::
    test_esrgan_discriminator applies to the same keys, and in float64 it equals oracle/srgan_oracle.py's forward plus autograd to 1e-12;
    ``content_loss`` equals oracle/srgan_oracle.content_loss_single plus autograd to 1e-12;
  * conditioning, on the oracle alone, of the cases the GPU tests use (x[:2] of the fixture; 2 x 3 x 48 x 32 for the content loss): with
    the discrete states of the EMULATED run replayed in all four runs, every compared tensor has E <= 1e-2 (f16) / 5e-2 (bf16) and
    8 G <= 1e-4, so that no 16-bit bound max(2 E, 8 G) of the GPU tests can exceed 2e-2 / 1e-1.  Measured, discriminator: E <= 2.8e-3 (f16, the logits; gradients <= 2.5e-3),
    <= 2.3e-2 (bf16; gradients <= 2.1e-2), 8 G <= 3.2e-5, against 6.1e-3 .. 9.6e-2 and 3.4e-2 .. 2.3e-1 for dx and the conv / BatchNorm
    gradients WITHOUT the replay -- why the GPU tests replay: a LeakyReLU unit whose pre-activation lies within a 16-bit rounding of zero
    (1 139 / 9 385 of 5 million units) takes the other slope, a factor of 5 on that element.  The forward is untouched by the replay (logits 2.8e-3 / 2.3e-2 either
    way).  ``classifier.2.bias``'s gradient, the sum of the logits' gradient, depends on no sign: its E, 1.6e-4 / 1.6e-3, is the rounding
    of sp.dl alone.  Content loss: d/dSR 1.1e-3 / 8.7e-3 with the three kinds of state replayed, 8.8e-2 / 2.9e-1 without; loss 7e-5 /
    2.5e-3;
  * the patterns the oracle derives from a stored map are the kernels': the pool routing equals F.max_pool2d(return_indices=True) on
    maps with exact ties between positive 16-bit values and all-zero windows (first maximum in row-major order, no gradient where the
    maximum is not positive);
  * the bounds see a subtle error: see test_*_bound_sees_a_subtle_error."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import srgan_oracle as O
from tests import esrgan_d_oracle as EO
from tests.util import checksum, load_golden, table

CAP = {"f16": 1e-2, "bf16": 5e-2}                    # the issue's conditions on E with the states replayed
G_CAP = 1e-4                                          # ... and on 8 G
STAGE = 5                                             # the stage the mutations hit: the middle of the stack
UPSTREAM = 2.5


def compared(res):
    """the keys of a run that the GPU test compares"""
    return [k for k in res if k != "loss" and not k.endswith("num_batches_tracked")]


def _rel_max(a, b):
    a, b = torch.as_tensor(np.asarray(a)).double(), torch.as_tensor(np.asarray(b)).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


# ---- the oracle is the reference's network ----
def test_discriminator_oracle_reproduces_the_reference(golden_dir):
    g = load_golden(golden_dir, "esrgan_discriminator.npz")
    x, state = EO.d_inputs(4)
    res = EO.discriminator(x, state, dtype=torch.float32, loss=EO.bce_ones)
    # the bounds of test_esrgan_discriminator's f32 mode, key by key
    assert _rel_max(res["logits"], g["train0_logits"]) < 1e-3 and _rel_max(res["logits"], g["train2_logits"]) < 1e-3
    assert abs(float(res["loss"]) - float(g["bce_ones"])) < 1e-3
    for k, want in table(g, "train0_statesum").items():
        assert np.allclose(checksum(res["state." + k]), want, rtol=1e-3, atol=1e-3 * abs(want[1]) + 1e-7), k
    seen = 0
    for key in g.files:
        if key.startswith("grad/"):
            e = EO.rel_l2(res["grad." + key[5:]], g[key])
        elif key.startswith("gradrows/"):
            e = EO.rel_l2(res["grad." + key[9:]][:2], g[key])
        else:
            continue
        seen += 1
        deep = any(t in key for t in ("features.26", "features.27", "classifier"))
        assert e < (1e-4 if deep else 2e-2), (key, e)
    assert seen == 12
    for k, want in table(g, "gsum").items():
        assert np.allclose(checksum(res["grad." + k]), want, rtol=2e-2, atol=5e-3 * abs(want[1]) + 1e-6), k
    assert len(table(g, "gsum")) == 33 == len(EO.d_param_names(state))
    assert EO.rel_l2(res["dx"], g["train2_dx"]) < 3e-2
    assert all(int(res["state.features.%d.num_batches_tracked" % (fi + 1)]) == 1 for fi in O.ESRGAN_D_CONVS[1:])


def test_discriminator_oracle_is_srgan_oracles_forward_plus_autograd():
    x, state = EO.d_inputs(2)
    res = EO.discriminator(x, state, loss=EO.bce_ones)
    P = {k: (v.double().clone().requires_grad_(True) if k in EO.d_param_names(state) else v.double().clone()) for k, v in state.items()}
    xl = x.double().clone().requires_grad_(True)
    logits = O.esrgan_discriminator_forward(xl, P, training=True)
    O.bce_with_logits_mean(logits, 1.0).backward()
    assert EO.rel_l2(res["logits"], logits) <= 1e-12 and EO.rel_l2(res["dx"], xl.grad) <= 1e-12
    for k in EO.d_param_names(state):
        assert EO.rel_l2(res["grad." + k], P[k].grad) <= 1e-12, k
    for k in state:
        if "running" in k:
            assert EO.rel_l2(res["state." + k], P[k]) <= 1e-12, k
    # its own signs replayed: the same numbers; d_logits in place of the loss: the same numbers
    own = EO.discriminator(x, state, loss=EO.bce_ones, signs=EO.stored_signs(res))
    d_logits = (torch.sigmoid(res["logits"]) - 1.0) / res["logits"].numel()
    alt = EO.discriminator(x, state, d_logits=d_logits, loss_scale=64.0)
    for k in compared(res):
        assert EO.rel_l2(own[k], res[k]) <= 1e-13 and EO.rel_l2(alt[k], res[k]) <= 1e-12, k


def test_content_loss_oracle_is_srgan_oracles_plus_autograd():
    sr, gt, P = EO.content_inputs()
    probe = {}
    res = EO.content_loss(sr, gt, P, upstream=UPSTREAM, probe=probe)
    so = sr.double().clone().requires_grad_(True)
    want = O.content_loss_single(so, gt.double(), {k: v.double() for k, v in P.items()}, EO.NODE, EO.MEAN, EO.STD)
    (UPSTREAM * want).backward()
    assert abs(float(res["loss"]) - float(want.detach())) <= 1e-12 * abs(float(want.detach())) and EO.rel_l2(res["dsr"], so.grad) <= 1e-12
    own = EO.content_loss(sr, gt, P, upstream=UPSTREAM, states=EO.stored_states(probe), loss_scale=64.0)
    assert EO.rel_l2(own["dsr"], res["dsr"]) <= 1e-13 and float(own["loss"]) == float(res["loss"])
    assert len(probe["maps"]) == 16 and len(probe["pre_pool"]) == 4 and tuple(probe["maps"][-1].shape) == (2, 512, 3, 2)


# ---- conditioning ----
@functools.lru_cache(maxsize=None)
def d_plain():
    x, state = EO.d_inputs(2)
    probes = {tag: {} for tag in ("f64", "f16", "bf16")}
    runs = {tag: EO.discriminator(x, state, loss=EO.bce_ones, probe=probes.get(tag), **EO.run_kw(tag)) for tag in ("f64", "f32", "f16", "bf16")}
    return runs, probes


@functools.lru_cache(maxsize=None)
def d_replayed(tag):
    """the float64, float32 and ``tag`` runs with the emulated ``tag`` run's own signs replayed"""
    x, state = EO.d_inputs(2)
    signs = EO.stored_signs(d_plain()[0][tag])
    return dict(EO.all_runs(EO.discriminator, x, state, loss=EO.bce_ones, signs=signs, tags=("f64", "f32", tag)), signs=signs)


C_KEYS = ("loss", "dsr")                              # ... of a content-loss run


def bounds(rep, tag, keys=None):
    """per compared tensor (E, G, the GPU test's bound max(2 E, 8 G)) of replayed runs"""
    out = {}
    for k in keys or compared(rep["f64"]):
        E, G = EO.rel_l2(rep[tag][k], rep["f64"][k]), EO.rel_l2(rep["f32"][k], rep["f64"][k])
        out[k] = (E, G, max(2 * E, 8 * G))
    return out


@pytest.mark.parametrize("tag", ["f16", "bf16"])
def test_discriminator_case_is_well_conditioned(tag):
    (plain, probes), rep = d_plain(), d_replayed(tag)
    b = bounds(rep, tag)
    flipped = sum(int((s != (p > 0)).sum()) for s, p in zip(rep["signs"], probes["f64"]["pre"]))
    units = sum(s.numel() for s in rep["signs"])
    print("ESRGAN D %s: %d of %d LeakyReLU units have another sign than in the float64 run" % (tag, flipped, units))
    worst_plain = worst_rep = 0.0
    for k, (E, G, bound) in b.items():
        e0 = EO.rel_l2(plain[tag][k], plain["f64"][k])
        print("ESRGAN D %-4s %-44s E %.3e (without the replay %.3e)  8G %.3e  bound %.3e" % (tag, k, E, e0, 8 * G, bound))
        assert 0 < E <= CAP[tag] and 0 <= 8 * G <= G_CAP, (k, E, G)
        if k == "dx" or k.startswith("grad.features"):
            worst_plain, worst_rep = max(worst_plain, e0), max(worst_rep, E)
        if not (k == "dx" or k.startswith("grad.")):
            assert e0 == E, k                                        # the forward is untouched by the replay
    # why replay: without it the input-side gradients' E is more than ten times larger, and past the cap
    assert worst_plain > 10 * worst_rep and worst_plain > CAP[tag], (worst_plain, worst_rep)
    E2 = b["grad.classifier.2.bias"][0]
    print("ESRGAN D %s: classifier.2.bias's gradient depends on no sign: E %.3e, the rounding of the logits' gradient alone" % (tag, E2))
    assert E2 == EO.rel_l2(plain[tag]["grad.classifier.2.bias"], plain["f64"]["grad.classifier.2.bias"]) <= float(torch.finfo(EO.EMULATE[tag]).eps)
    assert 0 < flipped < 1e-2 * units


@functools.lru_cache(maxsize=None)
def c_plain():
    sr, gt, P = EO.content_inputs()
    probes = {tag: {} for tag in ("f64", "f32", "f16", "bf16")}
    return {tag: EO.content_loss(sr, gt, P, upstream=UPSTREAM, probe=probes[tag], **EO.run_kw(tag)) for tag in probes}, probes


def c_runs(states, tags):
    sr, gt, P = EO.content_inputs()
    return EO.all_runs(EO.content_loss, sr, gt, P, upstream=UPSTREAM, states=states, tags=tags)


@functools.lru_cache(maxsize=None)
def c_replayed(tag):
    states = EO.stored_states(c_plain()[1][tag])
    return dict(c_runs(states, ("f64", "f32", tag)), states=states)


@pytest.mark.parametrize("tag", ["f16", "bf16"])
def test_content_loss_case_is_well_conditioned(tag):
    (plain, probes), rep = c_plain(), c_replayed(tag)
    b = bounds(rep, tag, C_KEYS)
    for k, (E, G, bound) in b.items():
        e0 = EO.rel_l2(plain[tag][k], plain["f64"][k])
        print("content loss %-4s %-4s E %.3e (without the replay %.3e)  8G %.3e  bound %.3e" % (tag, k, E, e0, 8 * G, bound))
        assert 0 < E <= CAP[tag] and 8 * G <= G_CAP, (k, E, G)
    assert EO.rel_l2(plain[tag]["dsr"], plain["f64"]["dsr"]) > 10 * b["dsr"][0]
    # replaying any two of the three kinds of state and not the third is not enough
    own = EO.stored_states(probes["f64"])
    for kind in ("relu", "route", "sign"):
        part = dict(rep["states"], **{kind: own[kind]})
        r = c_runs(part, ("f64",))["f64"]
        # (the float64 run with its own ``kind``, against the emulated run with the emulated one's: what a partial replay leaves)
        e = EO.rel_l2(rep[tag]["dsr"], r["dsr"])
        print("content loss %s: %s not replayed: E %.3e" % (tag, kind, e))
        assert e > 4 * b["dsr"][0], (kind, e)
    live = [float(m.double().mean()) for m in rep["states"]["relu"]]
    assert all(0.2 <= v <= 0.8 for v in live), live                  # both branches of every ReLU


# ---- the derived patterns are the kernels' ----
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_pool_routing_is_the_kernels_rule(dt):
    """csrc/resample.hip, maxpool2_relu_bwd_kernel: the first maximum in row-major order, zero gradient where it is not positive --
    which is what F.max_pool2d's backward does behind a ReLU.  On a map of few distinct 16-bit values: ties in most windows."""
    g = torch.Generator().manual_seed(6)
    z = (torch.randint(-3, 4, (2, 8, 12, 10), generator=g).float() * 0.3).to(dt).double()     # 7 values: exact ties, all-nonpositive windows
    z[0, 0, :4] = -1.0
    a = F.relu(z)
    route = EO.pool_route(a)
    w = EO.windows(a)
    ties = int(((w == w.max(-1, keepdim=True).values).sum(-1) > 1).sum())
    zero = int((w.max(-1).values == 0).sum())
    pos_ties = int((((w == w.max(-1, keepdim=True).values).sum(-1) > 1) & (w.max(-1).values > 0)).sum())
    assert ties > 100 and zero > 20 and pos_ties > 50, (ties, zero, pos_ties)
    _, idx = F.max_pool2d(a, 2, 2, return_indices=True)
    H, W = a.shape[2:]
    iy, ix = idx // W, idx % W
    assert torch.equal(route, (iy % 2) * 2 + ix % 2)
    assert not torch.equal(route, EO.pool_route(a, last=True))
    # ... and the gradient through the replayed ops is torch's own through relu + max_pool2d
    zl = z.clone().requires_grad_(True)
    dy = torch.randn(2, 8, 6, 5, generator=g, dtype=torch.float64)
    F.max_pool2d(F.relu(zl), 2, 2).backward(dy)
    zr = z.clone().requires_grad_(True)
    EO._MaxPoolRoute.apply(EO._ReLUMask.apply(zr, EO.positive(a)), route).backward(dy)
    assert torch.equal(zl.grad, zr.grad)
    assert float(zr.grad[0, 0, :4].abs().max()) == 0.0
    # the L1 sign: three states, 0 at exact ties
    b = a.clone()
    b[1] = a[1].flip(-1)
    s = EO.l1_sign(a, b)
    assert set(s.unique().tolist()) == {-1.0, 0.0, 1.0}


# ---- the bounds see a subtle error ----
def _report(what, moved, b16, bbf):
    """the largest ratios moved / bound over the compared tensors"""
    r16 = max((moved["f16"][k] / (4 * b16[k][2]), k) for k in b16)
    rbf = max((moved["bf16"][k] / bbf[k][2], k) for k in bbf)
    print("%-64s moves %-28s %.3e = %.1f x (4 x the f16 bound); %-28s %.3e = %.1f x the bf16 bound" %
          (what, r16[1], moved["f16"][r16[1]], r16[0], rbf[1], moved["bf16"][rbf[1]], rbf[0]))
    return r16[0], rbf[0]


@pytest.mark.parametrize("name", ["slope", "rstd_const"])
def test_discriminator_bound_sees_a_subtle_error(name):
    """One deliberate error in the float64 run (esrgan_d_oracle.MUTATIONS, at stage 5), signs replayed: at least one compared tensor
    moves past 4 x the f16 bound and past the bf16 bound.  Measured (moved / (4 x f16 bound), moved / bf16 bound): LeakyReLU' slope 0.25:
    5.4 / 2.8 (features.15.bias's gradient moves by 5.9e-2); rstd held constant: 5.7 / 2.8 (features.12.bias's, 6.5e-2) -- both pass
    the hand-set 1.8e-1 / 3e-1 of test_esrgan_discriminator unnoticed."""
    x, state = EO.d_inputs(2)
    moved = {}
    for tag in ("f16", "bf16"):
        rep = d_replayed(tag)
        mut = EO.discriminator(x, state, loss=EO.bce_ones, signs=rep["signs"], mutate={name: STAGE})
        moved[tag] = {k: EO.rel_l2(mut[k], rep["f64"][k]) for k in compared(mut)}
    r16, rbf = _report("ESRGAN D, stage %d: %s" % (STAGE, EO.MUTATIONS[name]), moved, bounds(d_replayed("f16"), "f16"), bounds(d_replayed("bf16"), "bf16"))
    assert r16 > 1.0 and rbf > 1.0, (r16, rbf)


@pytest.mark.parametrize("name", ["eps", "unbiased"])
def test_discriminator_f32_bound_sees_a_finer_error(name):
    """eps 1e-3 / the unbiased variance in stage 5: for the f32 mode, whose bound is 8 G (1e-5 .. 3e-5 for the tensors
    with more than one element).  Taken over dx and the gradients only.  Measured: both move every one of them past its 8 G -- eps by
    16 .. 294 times (features.0.bias .. features.15.bias), the unbiased variance by 2.1 .. 91 times."""
    x, state = EO.d_inputs(2)
    rep = d_replayed("f16")
    mut = EO.discriminator(x, state, loss=EO.bce_ones, signs=rep["signs"], mutate={name: STAGE})
    b = bounds(rep, "f16")
    ratios = sorted((EO.rel_l2(mut[k], rep["f64"][k]) / (8 * b[k][1]), k) for k in b if k == "dx" or k.startswith("grad."))
    several = [r for r in ratios if rep["f64"][r[1]].numel() > 1]                  # (a one-element tensor's G is anything down to zero)
    print("ESRGAN D, stage %d: %-64s moves dx and the gradients to %.1f (%s) .. %.1f (%s) x their 8 G" %
          (STAGE, EO.MUTATIONS[name], several[0][0], several[0][1], several[-1][0], several[-1][1]))
    assert several[-1][0] > 1.0, ratios


def _content_mutations(tag):
    """name -> the emulated ``tag`` run's states with one error"""
    states, probe = c_replayed(tag)["states"], c_plain()[1][tag]
    relu = list(states["relu"])
    relu[7] = torch.ones_like(relu[7])
    route = list(states["route"])
    route[0] = EO.pool_route(probe["pre_pool"][0], last=True)
    return {"relu_dropped": dict(states, relu=relu), "route_last": dict(states, route=route)}


CONTENT_MUTATIONS = {
    "relu_dropped": "features.16's ReLU mask (the middle of the chain) left out of the backward",
    "route_last": "the first pool routes to the LAST maximum of a window instead of the first",
}


@pytest.mark.parametrize("name", ["relu_dropped", "route_last"])
def test_content_loss_bound_sees_a_subtle_error(name):
    """The same on the VGG side, as edits of the replayed states.  The last maximum differs from the first only in windows whose largest
    stored values tie exactly and are positive: 13 of 49 152 windows of the first pool in the emulated f16 run, 89 in bf16.  Measured
    (moved / (4 x f16 bound), moved / bf16 bound): ReLU mask dropped 88 / 46; last maximum 2.4 / 4.1 (d/dSR moves by 2.1e-2 / 7.2e-2,
    under the hand-set 1.5e-1 / 4e-1 of test_differentiable_single_node_content_loss)."""
    moved = {}
    for tag in ("f16", "bf16"):
        mut = c_runs(_content_mutations(tag)[name], ("f64",))["f64"]
        moved[tag] = {k: EO.rel_l2(mut[k], c_replayed(tag)["f64"][k]) for k in C_KEYS}
    r16, rbf = _report("content loss: " + CONTENT_MUTATIONS[name], moved, bounds(c_replayed("f16"), "f16", C_KEYS), bounds(c_replayed("bf16"), "bf16", C_KEYS))
    assert r16 > 1.0 and rbf > 1.0, (r16, rbf)
    assert moved["f16"]["loss"] == 0.0                                # the forward is untouched
