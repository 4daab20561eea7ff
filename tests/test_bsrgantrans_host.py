"""Host-side checks of BSRGANtrans / bsrgantrans_x2 (no GPU: the library runs in dry-run mode, where every entry point validates its
arguments and launches nothing):

  * the float64 oracle (tests/bsrgantrans_oracle.py) against what the reference's own BSRGANtrans computed (tests/golden/
    bsrgantrans.npz, written by tests/golden/make_golden_bsrgantrans.py): SR to 1e-12, gradients to 1e-11 of the tensor's largest
    magnitude (measured: 3e-15 / 2e-15), ``transformer_layer.*`` gradients None;
  * keys, shapes and seeded values of the module against the reference's; deepcopy and pickle; every refusal;
  * the conditions under which the GPU bounds of tests/test_bsrgantrans_gpu.py mean something, on the oracle alone: 5-40 % of the SR
    pixels clamped, transformer_oracle's LayerNorm-variance, ReLU-liveness and softmax-entropy conditions, E and G finite and non-zero;
  * the plan at the training shape (8, 3, 60, 60), f16, train: the stand-alone encoder's lists at (8, 900, 64) as contiguous runs, one
    3x3 stride-2 forward, one class-4 data gradient, one (3, 2) weight gradient, upsamplingTrans in parity form; the gradient buckets;
    what an inference plan allocates."""
import copy
import math
import os
import pickle

import numpy as np
import pytest
import torch

from tests import bsrgantrans_oracle as BO
from tests.golden.make_golden import checksum


@pytest.fixture(scope="module")
def golden():
    with np.load(BO.FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture
def dry_run():
    from sr_gan_fd_amd import _abi as A
    A.set_dry_run(True)
    yield A
    A.set_dry_run(False)


def test_oracle_reproduces_the_reference(golden):
    assert os.path.getsize(BO.FIXTURE) < 1 << 20
    state = {k: v.double() for k, v in BO.case_inputs("fixture")[1].items()}
    # the rebuilt, edited parameters are the reference's: checksums of the seeded construction first (test_parameters_are_the_references)
    res = BO.generator(torch.from_numpy(golden["x"]), state, 2, d_out=torch.from_numpy(golden["dsr"]))
    rel = lambda a, want: float(np.abs(a - want).max() / np.abs(want).max())
    assert rel(res["out"].numpy(), golden["sr"]) <= 1e-12
    assert rel(res["dx"].numpy(), golden["dx"]) <= 1e-11
    seen = 0
    for k in BO.param_names(state):
        if "grad." + k in golden:
            assert rel(res[k].numpy(), golden["grad." + k]) <= 1e-11, k
        elif "gradsum." + k in golden:
            want = golden["gradsum." + k]
            assert np.abs(checksum(res[k]) - want).max() <= 1e-10 * max(1.0, np.abs(want).max()), k
        else:
            assert res[k] is None and k in set(str(n) for n in golden["grad_none"]), k
        seen += 1
    assert seen == 80 and len(golden["grad_none"]) == 12 and all(str(n).startswith("transformer_layer.") for n in golden["grad_none"])
    assert 0.05 <= float(golden["clamped_share"]) <= 0.40
    probe = {}
    BO.generator(torch.from_numpy(golden["x"]), state, 2, probe=probe)
    assert rel(probe["enc_src"][0].numpy(), golden["enc_src"]) <= 1e-12 and rel(probe["enc_out"][0].numpy(), golden["enc_out"]) <= 1e-12


def test_parameters_are_the_references(golden, capsys):
    from sr_gan_fd_amd import model as M
    torch.manual_seed(BO.SEED)
    m = M.bsrgantrans_x2(channels=64, growth_channels=32, num_rrdb=1)
    assert capsys.readouterr().out == "* BSRGAN TRANSFORMER 2x\n"
    got = m.state_dict()
    assert list(got) == [str(k) for k in golden["seeded.keys"]]
    for k, v in got.items():
        assert tuple(golden["seeded.shape." + k]) == tuple(v.shape), k
        assert np.abs(checksum(v) - golden["seeded.sum." + k]).max() <= 1e-9, k
    names = [n for n, _ in m.named_parameters()]
    order = ["conv1", "trunk", "downsamplingTrans", "transformer_layer", "transformer_encoder", "upsamplingTrans", "conv2", "upsampling1", "conv3", "conv4"]
    assert [n.split(".")[0] for n in names if n.split(".")[0] not in [x.split(".")[0] for x in names[:names.index(n)]]] == order
    assert isinstance(m, M.BSRGANtrans) and m.upscale_factor == 2 and m.channels == 64 and m.compute_dtype is None
    assert isinstance(m.transformer_layer, M.TransformerEncoderLayer) and isinstance(m.transformer_encoder, M.TransformerEncoder)
    assert "BSRGANtrans" in M.__all__ and "bsrgantrans_x2" in M.__all__ and M.__dict__["bsrgantrans_x2"] is M.bsrgantrans_x2
    assert hasattr(M.BSRGANtrans(num_rrdb=1), "upsampling2") and not hasattr(m, "upsampling2")


def test_copies_get_their_own_engine(dry_run):
    from sr_gan_fd_amd.engine import generator_engine
    m = BO.build_module()
    x = torch.rand(2, 3, 4, 6)
    assert m.dropout_masks() == {}
    m.train()
    assert m(x).shape == (2, 3, 8, 12)
    c, q = copy.deepcopy(m), pickle.loads(pickle.dumps(m))
    assert len(m.dropout_masks()) == 8 and c.dropout_masks() == {} and q.dropout_masks() == {}
    assert c(x).shape == q(x).shape == (2, 3, 8, 12)
    assert len({id(generator_engine(t)) for t in (m, c, q)}) == 3
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), q.state_dict().values()))
    eng = generator_engine(m)
    assert type(eng).__name__ == "TransGeneratorEngine" and eng.fp.total == sum((p.numel() + 3) // 4 * 4 for p in m.parameters())


def test_refusals(dry_run):
    from sr_gan_fd_amd import model as M, ops
    from sr_gan_fd_amd.trainer import GeneratorTrainer
    A = dry_run
    m = BO.build_module()
    for shape, text in (((2, 3, 5, 8), "even H and W"), ((2, 3, 6, 7), "even H and W"), ((ops.SEQ_ATTN_MAX_SEQ + 1, 3, 2, 2), "batch 129"),
                        ((2, 4, 6, 8), r"expects \(N, 3, H, W\)"), ((3, 6, 8), "4-D")):
        with pytest.raises(A.SrganfdError, match=text):
            m(torch.rand(*shape))
    with pytest.raises(A.SrganfdError, match="multiple of 32"):
        M.BSRGANtrans(channels=48, num_rrdb=1)                      # 12 channels a head, and no MFMA width
    with pytest.raises(A.SrganfdError, match="head size"):
        M.BSRGANtrans(channels=32, num_rrdb=1)                      # 8 channels a head
    with pytest.raises(A.SrganfdError, match="head size"):
        M.BSRGANtrans(channels=512, num_rrdb=1)                     # 128
    with pytest.raises(A.SrganfdError, match="multiples of 32"):
        M.BSRGANtrans(growth_channels=16, num_rrdb=1)(torch.rand(1, 3, 4, 4))
    # someone replaces the sub-modules: what check_layer refuses is refused here, before anything is packed
    bad = BO.build_module()
    bad.transformer_encoder.layers[1].norm_first = True
    with pytest.raises(A.SrganfdError, match="norm_first"):
        bad(torch.rand(1, 3, 4, 4))
    bad = BO.build_module()
    bad.transformer_encoder.norm = torch.nn.LayerNorm(64)
    with pytest.raises(A.SrganfdError, match="final norm"):
        bad(torch.rand(1, 3, 4, 4))
    bad = BO.build_module()
    bad.downsamplingTrans[0] = torch.nn.Conv2d(64, 64, 1)
    with pytest.raises(A.SrganfdError, match="downsamplingTrans.0.weight"):
        bad(torch.rand(1, 3, 4, 4))
    # the overwritten-activations case
    x = torch.rand(2, 3, 4, 4, requires_grad=True)
    first = m(x)
    m(x)
    with pytest.raises(A.SrganfdError, match="overwritten by a later forward"):
        first.sum().backward()
    with pytest.raises(A.SrganfdError, match="weight_decay"):
        GeneratorTrainer(m, lr=1e-4, weight_decay=1e-2)
    A.set_dry_run(False)
    with pytest.raises(A.SrganfdError, match="not on a GPU"):
        m(torch.rand(2, 3, 4, 4))


# ---- the conditions on the GPU cases, on the oracle alone ----
@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("name", list(BO.CASES))
def test_gpu_cases_are_well_conditioned(name, train):
    r = BO.eval_runs(name)
    x, state, d_out, up = r["x"], r["state"], r["d_out"], r["upscale"]
    B, _, H, W = x.shape
    if train:
        masks = BO.make_masks(state, B, (H // 2) * (W // 2), BO.P_TRAIN, seed=9)
        runs, probe = BO.all_runs(x, state, up, d_out, masks, BO.P_TRAIN), {}
        BO.generator(x, state, up, masks=masks, p=BO.P_TRAIN, probe=probe)
    else:
        runs, probe = r, r["probe"]
    share = float(BO.clamped(runs["f64"]["out"]).double().mean())
    assert 0.05 <= share <= 0.40, share                                # both branches of the clamp's derivative, without hiding the tail
    for k, ref in runs["f64"].items():
        if ref is None:
            continue
        for dt in ("f32", "f16", "bf16"):
            gap = BO.rel_l2(runs[dt][k], ref)
            assert math.isfinite(gap) and gap > 0, (dt, k, gap)
        assert BO.rel_l2(runs["f32"][k], ref) <= 1e-3, k
    for pre in ("layers.0.", "layers.1."):
        prob = probe[pre + "prob"]
        assert float((prob.sum(-1) - 1).abs().max()) < 1e-12
        if B > 1:
            ent = float(-(prob * torch.log(prob.clamp_min(1e-300))).sum(-1).mean()) / math.log(B)      # mean row entropy: 0 one-hot, 1 uniform
            # transformer_oracle's condition, 0.1 .. 0.9, for every case with scaled q and k rows (bsrgantrans_oracle.QK).  The fixture's
            # case keeps the reference run's recipe, under which the rows are near uniform (0.98 .. 0.999): there, not one-hot and not
            # exactly uniform is what can be asked, and the q / k gradients are covered by the other cases
            assert (0.1 <= ent < 1.0 - 1e-5) if name == "fixture" else (0.1 <= ent <= 0.9), (pre, ent)
        assert float(probe[pre + "var1"].min()) > 1e3 * BO.TO.EPS and float(probe[pre + "var2"].min()) > 1e3 * BO.TO.EPS, pre
        live = float((probe[pre + "hidden"] > 0).double().mean())
        assert 0.2 <= live <= 0.8, (pre, live)


# ---- the plan ----
def desc(it):
    """what an item launches, without its addresses"""
    if it.kind == "conv":
        a = it.args
        return ("conv", a.dtype, a.n, a.h_in, a.w_in, a.up, a.ksize, a.stride, a.pad, a.cin, a.cout, a.h_out, a.w_out, a.act, a.y_f32, a.out_classes,
                bool(a.r1.ptr), bool(a.r2.ptr), bool(a.mask.ptr), round(a.mask_slope, 6), bool(a.bias), a.x.planar, a.y.planar)
    if it.kind == "wgrad":
        return ("wgrad", it.plan.label, it.plan.flops, it.x.planar, it.dy.planar)
    if it.kind == "draw_masks":
        return ("draw_masks", tuple((tuple(t.shape), p) for t, p in it.masks))
    if it.kind == "ready":
        return ("ready", it.lo, it.hi)
    return (it.kind, getattr(it, "label", None), getattr(it, "work", None))


def find_run(seq, sub):
    hits = [i for i in range(len(seq) - len(sub) + 1) if seq[i:i + len(sub)] == sub]
    assert len(hits) == 1, hits
    return hits[0]


def test_plan_at_the_training_shape(dry_run):
    from sr_gan_fd_amd import model as M, ops
    from sr_gan_fd_amd.engine import generator_engine
    from sr_gan_fd_amd.transformer import transformer_engine
    A = dry_run
    m = BO.build_module().train()
    m.compute_dtype = torch.float16
    eng = generator_engine(m)
    eng.forward(torch.rand(8, 3, 60, 60), True)
    sp = eng._last
    enc = M.TransformerEncoder(M.TransformerEncoderLayer(64, 4), 2).train()
    enc.compute_dtype = torch.float16
    enc(torch.rand(8, 900, 64, requires_grad=True))
    sq = transformer_engine(enc)._last
    fw, bw = [desc(it) for it in sp.fw], [desc(it) for it in sp.bw]
    efw, ebw = [desc(it) for it in sq.fw], [desc(it) for it in sq.bw]
    assert fw[0][0] == "draw_masks" and fw[0] == efw[0] and len(fw[0][1]) == 8             # DrawMasks is the first forward item
    at = find_run(fw, efw[1:])
    assert sp.t_len == (len(efw) - 1, len(ebw))
    ab = find_run(bw, ebw)
    # ... identical except for the first layer's input gradient: the stand-alone engine launches it apart, in fp32, for a pass that wants
    # d src; here it follows the run, in the compute type, with LeakyReLU' of the stride-2 conv's output in its epilogue
    dx, edx = bw[ab + len(ebw)], desc(sq.dx_conv)
    names = ("kind", "dtype", "n", "h_in", "w_in", "up", "ksize", "stride", "pad", "cin", "cout", "h_out", "w_out", "act", "y_f32", "out_classes", "r1", "r2",
             "mask", "mask_slope", "bias", "x_planar", "y_planar")
    diff = {n: (a, b) for n, a, b in zip(names, dx, edx) if a != b}
    assert diff == {"y_f32": (0, 1), "mask": (True, False), "mask_slope": (0.2, edx[19])} or diff == {"y_f32": (0, 1), "mask": (True, False)}, diff
    # exactly one 3x3 stride-2 forward, from the trunk's planar buffer into NHWC, right in front of the run
    s2 = [d for d in fw if d[0] == "conv" and d[6:8] == (3, 2)]
    assert len(s2) == 1 and fw[at - 1] == s2[0] and s2[0][2:5] == (8, 60, 60) and s2[0][9:13] == (64, 64, 30, 30) and s2[0][13] == A.ACT_LRELU
    assert s2[0][21:] == (sp.planar, 0) and sp.planar == 1
    # one class-4 data gradient (2x2-tap classes over the 30 x 30 gradient, into the planar stacked-gradient buffer) and one (3, 2) weight gradient
    c4 = [d for d in bw if d[0] == "conv" and d[15] == 4 and d[6] == 2 and not d[20]]
    assert len(c4) == 1 and c4[0][2:5] == (8, 30, 30) and c4[0][21:] == (0, 1) and ops.CLASS4_ENABLED
    wg = [d for d in bw if d[0] == "wgrad" and "KS=3,S=2" in d[1]]
    assert len(wg) == 1 and wg[0][3:] == (1, 0)
    assert bw.index(wg[0]) == ab + len(ebw) + 1 and bw.index(c4[0]) == ab + len(ebw) + 2
    # upsamplingTrans in parity form: one class launch with a bias forward (30 x 30 -> 60 x 60), the 4x4 stride-2 data gradient backward
    assert fw[at + len(efw) - 1] == ("conv", A.F16, 8, 30, 30, 0, 2, 1, 0, 64, 64, 30, 30, A.ACT_LRELU, 0, 4, False, False, False, 0.2, True, 0, 0)
    assert bw[ab - 1][:13] == ("conv", A.F16, 8, 60, 60, 0, 4, 2, 1, 64, 64, 30, 30) and not bw[ab - 1][18] and bw[ab - 2][0] == "wgrad"
    # conv2's data gradient carries LeakyReLU' of upsamplingTrans's output
    assert bw[ab - 3][0] == "ready" and bw[ab - 4][:5] == ("conv", A.F16, 8, 60, 60) and bw[ab - 4][18] and bw[ab - 4][19] == 0.2
    assert sorted(m.dropout_masks()) == sorted("transformer_encoder.layers.%d.%s" % (i, s) for i in range(2) for s in BO.TO.SITES)
    assert m.dropout_masks()["transformer_encoder.layers.0.attn"].shape == (900, 4, 8, 8)


@pytest.mark.parametrize("num_rrdb", [1, 2])
def test_gradient_buckets_are_disjoint_and_cover_the_buffer(dry_run, num_rrdb):
    from sr_gan_fd_amd import ops
    from sr_gan_fd_amd.engine import generator_engine
    m = BO.build_module(num_rrdb)
    m.compute_dtype = torch.float16
    eng = generator_engine(m)
    eng.forward(torch.rand(2, 3, 8, 8), True)
    sp = eng._last
    ready = [(i, it.lo, it.hi) for i, it in enumerate(sp.bw) if isinstance(it, ops.Ready)]
    spans = sorted((lo, hi) for _, lo, hi in ready if hi > lo)
    assert spans[0][0] == 0 and spans[-1][1] == eng.fp.total and all(a[1] == b[0] for a, b in zip(spans[:-1], spans[1:])), spans
    off = eng.fp.off
    assert ready[0][1:] == (off("conv2.weight"), eng.fp.total)                               # from conv2 on: one contiguous tail
    assert ready[1][1:] == (off("downsamplingTrans.0.weight"), off("conv2.weight"))          # the stage, transformer_layer.* among it
    assert len(ready) == (3 if num_rrdb == 1 else 4)
    # the stage's bucket is announced before the first dense block's launches, after the stage's last launch
    first_block = min(i for i, it in enumerate(sp.bw) if it.kind in ("chain", "wgrad_partial", "wgrad_partial_batch") or getattr(it, "block", None) is not None)
    assert ready[1][0] < first_block
    # the flat gradient of this engine is zeroed: nothing writes transformer_layer.*'s range
    assert eng.fp.unwritten and len(eng.unused_params) == 12
    g = eng.fp.new_grad(torch.device("cpu"))
    assert float(g.abs().sum()) == 0.0


def test_inference_plan_allocates_no_backward_buffers(dry_run):
    from sr_gan_fd_amd.engine import generator_engine
    m = BO.build_module().eval()
    eng = generator_engine(m)
    with torch.no_grad():
        m(torch.rand(2, 3, 8, 8))
    sp = eng._last
    assert sp.token is None and getattr(sp, "bw", None) is None and sp.g_enc is None and sp.ln_ws is None and sp.t_wplans is None and not sp.masks
    for name in ("g_ut", "g_ds", "g_tmp", "dy", "dx0", "gA", "gB", "dsrp", "dxp", "wg_ws"):
        assert getattr(sp, name, None) is None, name
    a, b = sp.layers
    backward_only = ("dz2", "df", "dhid", "dy1", "dz1", "da", "datt", "dqkv", "dx")
    assert all(not hasattr(l, n) for l in (a, b) for n in backward_only)
    # one set of layer buffers for the stack: z, the statistics and lse are written (the kernels' outputs) and never read again
    assert all(getattr(a, n) is getattr(b, n) for n in ("qkv", "att", "a", "z1", "y1", "hid", "f", "z2", "lse", "mean1", "rstd1", "mean2", "rstd2"))
    assert a.y2 is not b.y2 and sp.enc_out.data_ptr() == b.y2.data_ptr()
    m.train()                                                      # dropout follows the module's mode: a plan with masks, even without gradients
    with torch.no_grad():
        m(torch.rand(2, 3, 8, 8))
    assert len(eng._last.masks) == 8 and eng._last.fw[0].kind == "draw_masks"
