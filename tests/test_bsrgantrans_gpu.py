"""BSRGANtrans / bsrgantrans_x2 on the GPU (sr_gan_fd_amd/engine_trans.py: the generator's engine with the stride-2 conv, the
transformer block and upsamplingTrans between trunk and conv2) against the torch-CPU restatement run in float64
(tests/bsrgantrans_oracle.py, pinned to the reference by tests/golden/bsrgantrans.npz), in f32, f16 and bf16, in eval mode and in train
mode with p = 0.1, the oracle replaying the module's own ``dropout_masks()``.  tests/test_bsrgantrans_host.py checks on the oracle alone
that the cases are well conditioned.

Cases (bsrgantrans_oracle.CASES; channels 64, growth 32): the fixture's shape (3, 6, 8); (1, 4, 4): one-token sequences and a 2 x 2 token
map; (2, 10, 6): token map 5 x 3, ragged parity classes; (5, 4, 6) with two RRDBs: odd batch and the second bucket marker; (2, 4, 4) at
x4 through the class: two tail stages.

Modules   (test_matches_oracle) SR, the image's gradient and every parameter gradient against the oracle in relative L2 under
          tests/test_transformer_gpu.py's rule -- f32: 8 G; f16 / bf16: max(2 E, 8 G), G the oracle's own float32-vs-float64 gap, E its
          gap with that type's rounding points, both computed live for the same masks.  test_matches_oracle prints every error / bound
          ratio; DESIGN.md 4h has the table.  ``transformer_layer.*`` gradients are None.
Exact     two forward + backward passes give the same bits; train mode with p = 0 gives eval's bits; the trunk's output buffer equals
          bsrgan_x2's over the same conv1 / trunk weights bit for bit; a stand-alone TransformerEncoder loaded with the generator's
          encoder state reproduces, from the engine's own downsample buffer, the engine's encoder output bit for bit.
Trainers  one GeneratorTrainer step at (3, 6, 8) <-> (3, 12, 16) and one GanTrainer step with UNetDiscriminatorAesrgan at (3, 8, 8) <->
          (3, 16, 16) (that discriminator takes multiples of 8 only), in train mode, masks replayed, against the oracle's steps: losses and SR under the rule above; parameters after Adam within 5e-3 of the
          tensor's range (tests/test_aesrgan_gpu.py's criterion); ``transformer_layer.*`` and its EMA copy bit-unchanged; the
          world-size and weight-decay refusals; GraphedStep; the drop-in Adam / AveragedModel.
MI355X    (DESIGN.md 4h has the table per case.)  f32: every tensor inside 8 G (SR 0.12-0.25 of it, gradients up to 0.58).  f16 / bf16: SR
          0.44-0.54 of max(2 E, 8 G) (an error equal to E); gradients 0.2-1.0 of it and, in 10 of the 20 sixteen-bit combinations, some
          tensors past it (fixture eval f16: one tensor at 1.015; up to 155 for conv4's gradients where the run has one SR pixel on the
          clamp and the emulated oracle none) -- E is mostly a few dozen LeakyReLU units whose pre-activation lies within a 16-bit rounding
          of zero, and which units flip differs between the emulated oracle and the kernels.  Those tensors pass the same rule with the
          stored pattern replayed (test_matches_oracle), at 0.36-0.64 of the smaller bound, and the flipped shares stay under their caps.
          Trainers: f32 loss 2e-9, SR 0.23, parameters and EMA 3.0e-4 of the range; f16 SR 0.45, ranged parameters 1.5e-3; bf16 0.51 /
          3.4e-3; GanTrainer scalars f32 4e-8..7e-8 relative, f16 3e-5..5e-5, bf16 4e-5..2e-4; SR 0.23 / 0.50 / 0.52; D's conv9.weight
          2e-8 / 8e-6 / 1.3e-4 of its range.
Deviations from the issue's plan, each with its reason where it is made: the GanTrainer pair; a scalar's bound has a floor (SCALAR_FLOOR,
          l1_floor, one unit roundoff for the discriminator's scalars in the 16-bit modes); the range criterion does not reach the
          constant-initialised tensors in the 16-bit modes (_check_params); the replayed comparison above.
"""
import copy
import functools

import pytest
import torch

from tests import bsrgantrans_oracle as BO

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def set_p(m, p):
    for layer in list(m.transformer_encoder.layers) + [m.transformer_layer]:
        layer.self_attn.dropout = p
        layer.dropout.p = layer.dropout1.p = layer.dropout2.p = p


def module(name, dt, train=False, p=BO.P_TRAIN):
    shape, num_rrdb, upscale, seed = BO.CASES[name]
    m = BO.build_module(num_rrdb, upscale, seed, qk=BO.case_qk(name))
    set_p(m, p)
    m.compute_dtype = dt
    return m.to(DEV).train(train)


def run(m, x, d_out):
    """forward + backward of the module: out, dx and every parameter gradient (None where the module has none), on the CPU"""
    m.zero_grad(set_to_none=True)
    xg = x.to(DEV).requires_grad_(True)
    out = m(xg)
    out.backward(d_out.to(DEV))
    torch.cuda.synchronize()
    res = {"out": out.detach().cpu(), "dx": xg.grad.cpu()}
    for k, prm in m.named_parameters():
        res[k] = None if prm.grad is None else prm.grad.detach().cpu().clone()
    return res


def stored_signs(m, sr):
    """bsrgantrans_oracle's ``signs`` of the module's last pass with a backward list: which units of every LeakyReLU were positive,
    read from the activations its plan stored, in forward order (the order of the oracle's "pre": the growth convs of every dense
    block, the stride-2 conv, upsamplingTrans, the upsampling layers, conv3), and which pixels of its result ``sr`` lie inside the clamp"""
    from sr_gan_fd_amd.engine import generator_engine
    eng = generator_engine(m)
    sp, C, G = eng._last, eng.Cc, eng.G
    nchw = lambda t: t.float().permute(0, 3, 1, 2)

    def planar(t):
        n, h, w, c = t.shape
        return t.view(n, c // 32, h, w, 32).permute(0, 1, 4, 2, 3).reshape(n, c, h, w).float() if sp.planar else nchw(t)
    out = []
    for i in range(eng.R):
        full = planar(sp.cat[i])
        out += [full[:, C + k * G: C + (k + 1) * G] > 0 for k in range(4)]
    out += [nchw(t) > 0 for t in [sp.ds, sp.ut] + list(sp.ups) + [sp.c3]]
    return {"lrelu": [t.cpu() for t in out], "inside": ~BO.clamped(sr.cpu())}


def flip_share(signs, pre):
    """share of LeakyReLU units whose sign is not the sign of the float64 oracle's pre-activation"""
    return sum(int((a != (b > 0)).sum()) for a, b in zip(signs, pre)) / sum(a.numel() for a in signs)


def flip_cap(own, units):
    """the cap on a share of flipped units: the emulated oracle's own share, three standard deviations of a count of that size, 8 units"""
    return own + 3 * (own / units) ** 0.5 + 8 / units


@functools.lru_cache(maxsize=None)
def train_runs(name, dt):
    """a train-mode pass of the module (seeded) and the oracle's four runs over the module's own masks"""
    r = BO.eval_runs(name)
    m = module(name, DTYPES[dt], train=True)
    torch.manual_seed(4)
    got = run(m, r["x"], r["d_out"])
    masks = {k: v.cpu() for k, v in m.dropout_masks().items()}
    assert sorted(masks) == sorted("transformer_encoder.layers.%d.%s" % (i, s) for i in range(2) for s in BO.TO.SITES)
    B, _, H, W = r["x"].shape
    assert masks["transformer_encoder.layers.0.attn"].shape == ((H // 2) * (W // 2), 4, B, B)
    assert masks["transformer_encoder.layers.1.dropout"].shape == (B, (H // 2) * (W // 2), 2048)
    for k, t in masks.items():
        assert t.dtype == torch.uint8 and int(t.max()) <= 1 and (t.numel() < 64 or 0.0 < float(t.float().mean()) < 1.0), k
    return got, dict(BO.all_runs(r["x"], r["state"], r["upscale"], r["d_out"], masks, BO.P_TRAIN), masks=masks, signs=stored_signs(m, got["out"]))


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("name", list(BO.CASES))
def test_matches_oracle(name, mode, dt):
    if mode == "eval":
        runs = BO.eval_runs(name)
        m = module(name, DTYPES[dt])
        got = run(m, runs["x"], runs["d_out"])
        masks, signs = None, stored_signs(m, got["out"])
    else:
        got, runs = train_runs(name, dt)
        masks, signs = runs["masks"], runs["signs"]
    ref, bad = runs["f64"], []
    assert set(got) == set(ref)
    for k in ref:
        if ref[k] is None:
            assert got[k] is None and k.startswith("transformer_layer."), k
            continue
        assert got[k] is not None and got[k].shape == ref[k].shape and got[k].dtype == torch.float32, k
        err, G = BO.rel_l2(got[k], ref[k]), BO.rel_l2(runs["f32"][k], ref[k])
        if dt == "f32":
            bound, what = 8 * G, "8G"
        else:
            E = BO.rel_l2(runs[dt][k], ref[k])
            bound, what = max(2 * E, 8 * G), "max(2E, 8G)"
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        print("%-9s %-5s %-4s %-52s err %.3e  %s %.3e  ratio %.3f  (to the emulated run %.3e)" %
              (name, mode, dt, k, err, what, bound, ratio, BO.rel_l2(got[k], runs[dt][k])))
        if not err <= bound:
            bad.append((k, err, bound))
    # a LeakyReLU pre-activation within a 16-bit rounding of zero (an SR value within one of 0 or 1) has one state in the float64 run and
    # may have the other in a 16-bit one; its derivative is then 1 against 0.2 (1 against 0).  A few dozen such units of 140 000 are most
    # of E (the fixture in f16: 25 units, E 3 % with them and 0.8 % without), and WHICH units flip differs between the emulated oracle and
    # the kernels.  The bound is not widened for that: the share of flipped units is capped, and a tensor that misses the rule is held
    # to the same rule against the same oracle with the pattern the GPU run stored replayed in the derivatives of all four runs (the
    # forward is untouched), under the smaller of the two bounds
    x, state, d_out, up = BO.case_inputs(name)
    p = BO.P_TRAIN if mode == "train" else 0.0
    probe = {}
    BO.generator(x, state, up, masks=masks, p=p, probe=probe)
    pre64 = probe["pre"]
    units, pixels = sum(a.numel() for a in signs["lrelu"]), ref["out"].numel()
    if dt == "f32":
        own_l = own_c = 0.0
    else:
        pe = {}
        own_c = float((BO.clamped(BO.generator(x, state, up, masks=masks, p=p, probe=pe, emulate=DTYPES[dt])["out"]) != BO.clamped(ref["out"])).double().mean())
        own_l = flip_share([t > 0 for t in pe["pre"]], pre64)
    mine_l, mine_c = flip_share(signs["lrelu"], pre64), float((signs["inside"] == BO.clamped(ref["out"])).double().mean())
    print("%-9s %-5s %-4s states that differ from the float64 oracle's: LeakyReLU units %.2e (the emulated oracle's own %.2e, cap %.2e), clamped SR "
          "pixels %.2e (own %.2e, cap %.2e)" % (name, mode, dt, mine_l, own_l, flip_cap(own_l, units), mine_c, own_c, flip_cap(own_c, pixels)))
    assert mine_l <= flip_cap(own_l, units) and mine_c <= flip_cap(own_c, pixels)
    if bad:
        rep = BO.all_runs(x, state, up, d_out, masks, p, signs=signs)
        still = []
        for k, err, bound in bad:
            e2, G2 = BO.rel_l2(got[k], rep["f64"][k]), BO.rel_l2(rep["f32"][k], rep["f64"][k])
            b2 = min(bound, 8 * G2 if dt == "f32" else max(2 * BO.rel_l2(rep[dt][k], rep["f64"][k]), 8 * G2))
            print("%-9s %-5s %-4s %-52s missed the rule (err %.3e, bound %.3e); states replayed: err %.3e  bound %.3e  ratio %.3f" %
                  (name, mode, dt, k, err, bound, e2, b2, e2 / b2))
            if not e2 <= b2:
                still.append((k, e2, b2))
        bad = still
    assert not bad, bad


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", ["fixture", "odd_batch"])
def test_exactness(name, dt):
    r = BO.eval_runs(name)
    m = module(name, DTYPES[dt])
    a, b = run(m, r["x"], r["d_out"]), run(m, r["x"], r["d_out"])
    same = lambda s, t: (s is None and t is None) or torch.equal(s, t)
    for k in a:
        assert same(a[k], b[k]), "two runs differ in " + k
    assert all((a[k] is None) == k.startswith("transformer_layer.") for k in a)
    c = run(module(name, DTYPES[dt], train=True, p=0.0), r["x"], r["d_out"])              # train mode, p = 0: no masks, eval's bits
    for k in a:
        assert same(a[k], c[k]), "train mode with p = 0 differs from eval mode in " + k
    m.train()                                                                             # p = 0.1: seeded masks, two runs agree
    torch.manual_seed(8)
    d = run(m, r["x"], r["d_out"])
    torch.manual_seed(8)
    e = run(m, r["x"], r["d_out"])
    assert not torch.equal(a["out"], d["out"])
    for k in d:
        assert same(d[k], e[k]), "two seeded train-mode runs differ in " + k
    with torch.no_grad():                                                                 # no gradient wanted: dropout follows the module's mode all the same
        torch.manual_seed(8)
        assert torch.equal(m(r["x"].to(DEV)).cpu(), d["out"])
        m.eval()
        assert torch.equal(m(r["x"].to(DEV)).cpu(), a["out"])                             # the inference plan: eval's bits


@pytest.mark.parametrize("dt", list(DTYPES))
def test_trunk_and_block_exactness(dt):
    from sr_gan_fd_amd import model as M
    from sr_gan_fd_amd.engine import generator_engine
    r = BO.eval_runs("odd_map")
    m = module("odd_map", DTYPES[dt])
    x = r["x"].to(DEV)
    plain = M.bsrgan_x2(num_rrdb=1)
    plain.load_state_dict({k: v for k, v in m.state_dict().items() if k in plain.state_dict()})
    plain.compute_dtype = DTYPES[dt]
    plain = plain.to(DEV).eval()
    xg = x.clone().requires_grad_(True)
    m(xg)
    plain(x.clone().requires_grad_(True))
    sp, sq = generator_engine(m)._last, generator_engine(plain)._last
    R = generator_engine(m).R
    # (channels [0, C) of the buffer: the rest would hold the growth convs of a block that does not exist)
    first = lambda t: t.view(t.shape[0], -1, t.shape[1], t.shape[2], 32)[:, :2] if sp.planar else t[..., :64]
    assert sp.planar == sq.planar and torch.equal(first(sp.catb(R)), first(sq.catb(R))), "the trunk's output buffers differ"
    # the block: a stand-alone encoder with the generator's encoder state, from the engine's own downsample buffer
    enc = M.TransformerEncoder(M.TransformerEncoderLayer(64, 4), 2)
    enc.load_state_dict(m.transformer_encoder.state_dict())
    enc.compute_dtype = DTYPES[dt]
    enc = enc.to(DEV).eval()
    B, h, w, C = sp.ds.shape
    with torch.no_grad():
        out = enc(sp.ds.float().view(B, h * w, C))
    assert torch.equal(out, sp.enc_out.float().view(B, h * w, C)), "the encoder inside the generator is not the stand-alone encoder"
    with torch.no_grad():                                                                 # ... and on the inference plan
        m(x)
    sp = generator_engine(m)._last
    assert getattr(sp, "g_enc", None) is None and not sp.masks and torch.equal(out, sp.enc_out.float().view(B, h * w, C))


# ---- trainers ----
HYPER = dict(lr=1e-4, betas=(0.9, 0.99), eps=1e-4)
GAN = dict(g_lr=5e-5, d_lr=1e-5, betas=(0.9, 0.999), eps=1e-4, pixel_weight=10.0, adversarial_weight=0.1)
RANGE_TOL = 5e-3                 # tests/test_aesrgan_gpu.py: parameters after Adam within this fraction of the tensor's range
# a logged scalar is ONE fp32 number: the float32 oracle's gap G to the float64 one is then anything between 0 and a unit roundoff, by
# chance, and 8 G no bound at all.  A scalar's bound is at least 2 unit roundoffs of fp32: one for the rounding of the kernel's result,
# one for the float32 oracle's (measured: 2e-9 .. 7e-8)
SCALAR_FLOOR = 2 * 2.0 ** -24
# float16 trainers start, as torch's GradScaler does, at a loss scale of 65536, at which the first steps of this 8-times-scaled network
# overflow and are skipped (parameters unchanged: nothing to compare); the compared step starts at a scale it does not overflow at
LOSS_SCALE = 256.0
t64 = lambda v: v.detach().double().cpu() if torch.is_tensor(v) else torch.tensor(float(v), dtype=torch.float64)      # noqa: E731


def rule(dt, got, ref, f32, emu, floor=0.0):
    """(error, bound) of tests/test_transformer_gpu.py's rule: f32 8 G; 16-bit max(2 E, 8 G)"""
    want = t64(ref)
    G = BO.rel_l2(t64(f32), want)
    bound = 8 * G if dt == "f32" else max(2 * BO.rel_l2(t64(emu), want), 8 * G)
    return BO.rel_l2(t64(got), want), max(bound, SCALAR_FLOOR if want.dim() == 0 else 0.0, floor)


def l1_floor(weight, sr_bound, sr_ref, loss_ref):
    """what the SR's bound allows the pixel loss: weight * mean|sr - gt| is weight-Lipschitz in the SR's root mean square, so a relative
    L2 error ``sr_bound`` of the SR moves it by at most weight * sr_bound * rms(sr).  (A scalar's own E is the mean of signed errors:
    by chance anything down to zero.)"""
    return weight * sr_bound * float(sr_ref.double().pow(2).mean().sqrt()) / abs(float(loss_ref))


def _gt(name="fixture"):
    x = BO.eval_runs(name)["x"]
    return torch.rand(x.shape[0], 3, 2 * x.shape[2], 2 * x.shape[3], generator=torch.Generator().manual_seed(77))


def _range_err(got, want):
    return float((got.double().cpu() - want.double()).abs().max() / (want.double().max() - want.double().min()).clamp_min(1e-30))


def _check_params(tag, dt, lr, state_after, flat_ema, fp, want, want_ema, before):
    """Parameters after Adam and their EMA copy within RANGE_TOL of the tensor's range (the issue's criterion; for a weight tensor of
    range 0.04 and more one step of 1e-4 cannot miss it).  In f32 it is asserted for ALL tensors (3.0e-4).  In the 16-bit modes it is
    asserted for the tensors that HAVE a range.  A tensor initialised to one constant (the conv biases at 0, conv4.bias, LayerNorm's
    weights and biases) has, after one step, no range but the step itself -- lr g / (|g| + eps), which for an element whose gradient is
    below the 16-bit gradient error (3 % of the tensor's norm) takes either sign.  For those the figure is PRINTED (f16 1.07 lr, bf16
    1.25 lr); the ``<= 2 lr`` beside it cannot fail and checks only that the tensor is finite and moved by no more than a step.  In the
    16-bit modes these tensors are covered by their gradients (test_matches_oracle) and by the f32 run of this test, not by this
    criterion."""
    worst, const = (0.0, ""), (0.0, "")
    ema = dict(zip(fp.names, fp.grad_views(flat_ema)))
    for which, got_d, want_d in (("", state_after, want), ("ema ", ema, want_ema)):
        for k, v in want_d.items():
            if k not in got_d or not v.is_floating_point():
                continue
            if k.startswith("transformer_layer."):
                assert torch.equal(got_d[k].cpu(), before[k]), which + k + " moved"
            elif dt != "f32" and float(before[k].max() - before[k].min()) == 0.0:
                const = max(const, (float((got_d[k].double().cpu() - v.double()).abs().max()) / lr, which + k))
            else:
                worst = max(worst, (_range_err(got_d[k], v), which + k))
    print("%s parameters after Adam and their EMA copy: worst |got - want| / range %.3e (%s), tolerance %.1e; constant-initialised tensors: "
          "worst |got - want| %.3f lr (%s)" % (tag, worst[0], worst[1], RANGE_TOL, const[0], const[1]))
    assert worst[0] <= RANGE_TOL and const[0] <= 2.0, (worst, const)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_generator_trainer_step_vs_oracle(dt):
    from sr_gan_fd_amd.trainer import GeneratorTrainer
    r = BO.eval_runs("fixture")
    gt = _gt()
    m = module("fixture", DTYPES[dt], train=True)
    before = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    tr = GeneratorTrainer(m, ema_decay=0.999, **HYPER)
    tr.scaler.scale = LOSS_SCALE
    torch.manual_seed(4)
    loss = float(tr.step(r["x"].to(DEV), gt.to(DEV)).item())
    assert tr.scaler.n_skipped == 0
    masks = {k: v.cpu() for k, v in m.dropout_masks().items()}
    runs = {}
    for tag, kw in (("f64", {}), ("f32", dict(dtype=torch.float32)), (dt, dict(emulate=DTYPES[dt]))):
        if tag in runs:
            continue
        ft = kw.get("dtype", torch.float64)
        G = {k: v.to(ft).clone() for k, v in r["state"].items()}
        ema = {}
        l, sr, n = BO.g_only_step(G, BO.O.AdamState(G, BO.param_names(G)), ema, 0, r["x"], gt, upscale=2, masks=masks, p=BO.P_TRAIN, **HYPER, **kw)
        runs[tag] = dict(loss=l, sr=sr, G=G, ema=ema)
    ref = runs["f64"]
    sr_bound = rule(dt, tr.sr, ref["sr"], runs["f32"]["sr"], runs[dt]["sr"])[1]
    for what, got, key in (("loss", loss, "loss"), ("sr", tr.sr, "sr")):
        err, bound = rule(dt, got, ref[key], runs["f32"][key], runs[dt][key], l1_floor(1.0, sr_bound, ref["sr"], ref["loss"]) if key == "loss" and dt != "f32" else 0.0)
        print("GeneratorTrainer %-4s %-4s err %.3e bound %.3e ratio %.3f" % (dt, what, err, bound, err / bound))
        assert err <= bound, (what, err, bound)
    _check_params("GeneratorTrainer " + dt, dt, HYPER["lr"], m.state_dict(), tr.opt.ema, tr.eng.fp, ref["G"], ref["ema"], before)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_gan_trainer_step_vs_oracle(dt):
    from sr_gan_fd_amd import model as M
    from sr_gan_fd_amd.gan import GanTrainer
    r = BO.eval_runs("fixture")
    # UNetDiscriminatorAesrgan takes heights and widths that are multiples of 8 only (engine_a.py), so the fixture's (3, 6, 8) <-> (3, 12, 16)
    # cannot pass through it: the same network on (3, 8, 8) <-> (3, 16, 16), the nearest pair it accepts
    g8 = torch.Generator().manual_seed(78)
    x, gt = torch.rand(3, 3, 8, 8, generator=g8), torch.rand(3, 3, 16, 16, generator=g8)
    torch.manual_seed(0)
    d = M.uNetDiscriminatorAesrgan()
    D0 = {k: v.detach().clone() for k, v in d.state_dict().items()}
    m = module("fixture", DTYPES[dt], train=True)
    d.compute_dtype = DTYPES[dt]
    d = d.to(DEV).train()
    before = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    tr = GanTrainer(m, d, None, **GAN)
    tr.scaler.scale = LOSS_SCALE
    torch.manual_seed(4)
    s = tr.step(x.to(DEV), gt.to(DEV)).cpu()
    assert tr.scaler.n_skipped == 0
    masks = {k: v.cpu() for k, v in m.dropout_masks().items()}
    runs = {}
    for tag, kw in (("f64", {}), ("f32", dict(dtype=torch.float32)), (dt, dict(emulate=DTYPES[dt]))):
        if tag in runs:
            continue
        ft = kw.get("dtype", torch.float64)
        G = {k: v.to(ft).clone() for k, v in r["state"].items()}
        D = {k: (v.to(ft) if v.is_floating_point() else v).clone() for k, v in D0.items()}
        ema = {}
        out = BO.gan_step(G, D, BO.O.AdamState(G, BO.param_names(G)), BO.O.AdamState(D, BO.O.d_param_names(D)), ema, 0, x, gt, upscale=2,
                          masks=masks, p=BO.P_TRAIN, **GAN, **kw)
        runs[tag] = dict(out=out, G=G, D=D, ema=ema)
    ref = runs["f64"]
    got = {"d_loss_hr": s[0], "d_loss_sr": s[1], "pixel_loss": s[2], "adversarial_loss": s[3], "d_gt_probability": s[4], "d_sr_probability": s[5],
           "sr": tr.sr.cpu()}
    sr_bound = rule(dt, got["sr"], ref["out"]["sr"], runs["f32"]["out"]["sr"], runs[dt]["out"]["sr"])[1]
    for k, v in got.items():
        # 16-bit: the oracle emulates the generator's rounding points; the discriminator's own 16-bit rounding is not in E, so the logged
        # scalars that pass through it get one unit roundoff of the type (f16 4.9e-4, bf16 3.9e-3; measured f16 3e-5 .. 5e-5) where that
        # is the larger bound, and the pixel loss what the SR's bound allows it (l1_floor)
        unit = float(torch.finfo(DTYPES[dt]).eps) / 2
        floor = 0.0 if k == "sr" or dt == "f32" else (l1_floor(GAN["pixel_weight"], sr_bound, ref["out"]["sr"], ref["out"][k]) if k == "pixel_loss" else unit)
        err, bound = rule(dt, v, ref["out"][k], runs["f32"]["out"][k], runs[dt]["out"][k], floor)
        print("GanTrainer %-4s %-18s err %.3e bound %.3e ratio %.3f" % (dt, k, err, bound, err / bound))
        assert err <= bound, (k, err, bound)
    _check_params("GanTrainer " + dt, dt, GAN["g_lr"], m.state_dict(), tr.g_opt.ema, tr.ge.fp, ref["G"], ref["ema"], before)
    e_d = _range_err(d.conv9.weight.detach(), ref["D"]["conv9.weight"])
    print("GanTrainer %s D conv9.weight after Adam: %.3e of its range" % (dt, e_d))
    assert e_d <= RANGE_TOL


def test_trainer_refusals():
    import torch.distributed as dist
    from sr_gan_fd_amd import _abi as A, model as M
    from sr_gan_fd_amd.gan import GanTrainer
    from sr_gan_fd_amd.trainer import GeneratorTrainer
    m = module("fixture", torch.float16, train=True)
    d = M.uNetDiscriminatorAesrgan().to(DEV)
    with pytest.raises(A.SrganfdError, match="weight_decay"):
        GeneratorTrainer(m, weight_decay=1e-4, **HYPER)
    with pytest.raises(A.SrganfdError, match="weight_decay"):
        GanTrainer(m, d, None, weight_decay=1e-4)

    class TwoRanks:                      # stands in for a process group of two ranks: the trainers ask only for its size
        pass
    real = dist.get_world_size
    dist.get_world_size = lambda pg=None: 2 if isinstance(pg, TwoRanks) else real(pg)
    try:
        with pytest.raises(A.SrganfdError, match="data-parallel"):
            GeneratorTrainer(m, process_group=TwoRanks(), **HYPER)
        with pytest.raises(A.SrganfdError, match="data-parallel"):
            GanTrainer(m, d, None, process_group=TwoRanks())
    finally:
        dist.get_world_size = real
    with pytest.raises(A.SrganfdError, match="even H and W"):
        GeneratorTrainer(m, **HYPER).step(torch.rand(2, 3, 5, 8, device=DEV), torch.rand(2, 3, 10, 16, device=DEV))


def test_graphed_step():
    from sr_gan_fd_amd.graph import GraphedStep
    from sr_gan_fd_amd.trainer import GeneratorTrainer
    gen = torch.Generator().manual_seed(5)
    data = [(torch.rand(3, 3, 6, 8, generator=gen).to(DEV), torch.rand(3, 3, 12, 16, generator=gen).to(DEV)) for _ in range(4)]
    me, mg = module("fixture", torch.float16, train=True, p=0.0), module("fixture", torch.float16, train=True, p=0.0)
    te, tg = GeneratorTrainer(me, ema_decay=0.999, **HYPER), GeneratorTrainer(mg, ema_decay=0.999, **HYPER)
    te.opt.use_device_step()             # the step count on the device in both: the same Adam kernel, so the same bits
    for _ in range(2):
        te.step(*data[0])
    step = GraphedStep(tg, *data[0], warmup=2)
    for lr, gt in data[1:]:
        le, lg = te.step(lr, gt).clone(), step(lr, gt).clone()
        assert torch.equal(le, lg) and torch.equal(te.sr, tg.sr)
    torch.cuda.synchronize()
    assert torch.equal(te.flat, tg.flat) and torch.equal(te.opt.ema, tg.opt.ema), "a replay does not give the eager step's bits"
    # p = 0.1: every replay draws its own masks
    mp = module("fixture", torch.float16, train=True)
    tp = GeneratorTrainer(mp, ema_decay=0.999, **HYPER)
    stepp = GraphedStep(tp, *data[0], warmup=2)
    seen = []
    for _ in range(2):
        loss = stepp(*data[1])
        torch.cuda.synchronize()
        seen.append({k: v.cpu() for k, v in mp.dropout_masks().items()})
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(tp.sr).all()) and bool(torch.isfinite(tp.flat).all())
    assert any(not torch.equal(seen[0][k], seen[1][k]) for k in seen[0]), "two replays read the same masks"


def test_dropin_adam_and_averaged_model_take_a_step():
    from sr_gan_fd_amd import optim as O, swa_utils as S
    from torch.optim.swa_utils import AveragedModel as TorchAveraged
    ema_fn = lambda a, p, n: (1 - 0.999) * a + 0.999 * p          # noqa: E731
    r = BO.eval_runs("fixture")
    gt = _gt().to(DEV)
    res = {}
    for kind in ("torch", "ours"):
        m = module("fixture", torch.float32, train=True, p=0.0)
        opt = (torch.optim.Adam if kind == "torch" else O.Adam)(m.parameters(), 1e-4, (0.9, 0.99), 1e-4, 0.0)
        ema = (TorchAveraged if kind == "torch" else S.AveragedModel)(m, avg_fn=ema_fn)
        for _ in range(2):
            m.zero_grad(set_to_none=True)
            torch.nn.functional.l1_loss(m(r["x"].to(DEV)), gt).backward()
            opt.step()
            ema.update_parameters(m)
        with torch.no_grad():
            sr = ema(r["x"].to(DEV))                   # the EMA copy has its own engine, in eval or train mode as the module was
        res[kind] = (m, ema, sr, opt)
    (mt, et, st, _), (mo, eo, so, oo) = res["torch"], res["ours"]
    # the fused whole-network paths are the ones taken: the 12 None gradients of transformer_layer.* are the engine's unread parameters
    # (flat.engine_grad_span), whose range of the flat gradient is zero
    assert oo.flat_steps == 2 and eo.flat_updates == 2, (oo.flat_steps, eo.flat_updates)
    fresh = module("fixture", torch.float32, train=True, p=0.0)
    for k, v in mo.state_dict().items():
        if k.startswith("transformer_layer."):
            assert torch.equal(v, fresh.state_dict()[k]), k + " moved"
    close = lambda a, b: torch.allclose(a.float().cpu(), b.float().cpu(), rtol=2e-5, atol=1e-7)
    for (k, a), (_, b) in zip(mt.state_dict().items(), mo.state_dict().items()):
        assert close(a, b), k
    for (k, a), (_, b) in zip(et.state_dict().items(), eo.state_dict().items()):
        assert close(a, b), k
    # (the EMA copy's SR: tests/test_dropin_optim_gpu.py's tolerance for it -- the fused step and torch's differ in the last bits of the parameters)
    assert torch.allclose(st.cpu(), so.cpu(), rtol=1e-4, atol=1e-5) and mo.transformer_layer.linear1.weight.grad is None
    assert copy.deepcopy(mo)(r["x"].to(DEV)).shape == (3, 3, 12, 16)
