"""Host-side checks of TransformerEncoderLayer / TransformerEncoder (no GPU: the library runs in dry-run mode, where every entry
point validates its arguments and launches nothing):

  * the float64 oracle (tests/transformer_oracle.py) against what the reference's own BSRGANtrans computed around its
    ``transformer_encoder`` (tests/golden/transformer.npz, written by tests/golden/make_golden_transformer.py) -- this pins the
    orientation: the sequence axis is the batch of images;
  * the oracle with the three module-level keep-masks against a float64 nn.TransformerEncoderLayer in train mode (its masks recovered
    by forward hooks on its Dropout modules, ``self_attn.dropout`` = 0), and the attention-probability site against the plain formula
    softmax -> mask -> . V;
  * keys, shapes and seeded values of the two classes; every refusal; the calls a forward + backward makes at the consumer's shape;
  * the conditions under which the GPU bounds of tests/test_transformer_gpu.py mean something, on the oracle alone: the yardstick
    E <= 0.05 (f16) / 0.15 (bf16), softmax rows neither one-hot nor uniform (mean row entropy within 0.1 .. 0.9 of log S), LayerNorm
    variances far above eps, between 0.2 and 0.8 of the ReLU units live, every keep-mask mixed."""
import copy
import math
import os
import pickle
import warnings

import numpy as np
import pytest
import torch

from tests import transformer_oracle as TO
from tests.golden.make_golden import checksum

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transformer.npz")


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


def _stack(E=64, heads=4, F=2048, layers=2, dropout=0.1):
    from sr_gan_fd_amd import model as M
    return M.TransformerEncoder(M.TransformerEncoderLayer(E, heads, F, dropout), layers)


def test_oracle_reproduces_the_reference(golden):
    assert os.path.getsize(FIXTURE) < 1 << 20
    state = {k[len("state."):]: torch.from_numpy(v.astype(np.float64)) for k, v in golden.items() if k.startswith("state.")}
    S, N, E, B, h, w = (int(v) for v in golden["orientation"])
    assert (S, N) == (B, h * w)                                      # the sequence axis is the batch, every pixel a sequence
    src, dout = torch.from_numpy(golden["src"]), torch.from_numpy(golden["dout"])
    assert src.shape == (S, N, E)
    res = TO.encoder(src, state, int(golden["nhead"]), d_out=dout)
    rel = lambda a, want: float(np.abs(a - want).max() / np.abs(want).max())
    assert rel(res["out"].numpy(), golden["out"]) <= 1e-12
    assert rel(res["dsrc"].numpy(), golden["dsrc"]) <= 1e-11
    seen = 0
    for k in state:
        if "grad." + k in golden:
            assert rel(res[k].numpy(), golden["grad." + k]) <= 1e-11, k
        else:
            want = golden["gradsum." + k]
            assert np.abs(checksum(res[k]) - want).max() <= 1e-10 * max(1.0, np.abs(want).max()), k
        seen += 1
    assert seen == 24
    # transposing the two token axes -- what a batch_first reading of the same tensor would compute -- is another function
    other = TO.encoder(src.transpose(0, 1).contiguous(), state, int(golden["nhead"]))["out"].transpose(0, 1)
    assert rel(other.numpy(), golden["out"]) > 1e-3


def test_oracle_matches_torch_in_train_mode():
    """dropout1, the feed-forward dropout and dropout2 replayed from torch's own masks"""
    heads, src, state, d_out = TO.case_inputs("odd_seq")
    S, N, E, _, F, _ = TO.CASES["odd_seq"]
    layer = torch.nn.TransformerEncoderLayer(E, heads, F, dropout=TO.P_TRAIN).double()
    layer.load_state_dict({k[len("layers.0."):]: v.double() for k, v in state.items()})
    layer.self_attn.dropout = 0.0
    layer.train()
    masks = {}
    for site in ("dropout1", "dropout", "dropout2"):
        # (an input that is exactly zero -- a dead ReLU unit -- reads as kept: its mask bit changes neither the output nor any gradient)
        getattr(layer, site).register_forward_hook(lambda m, i, o, site=site: masks.__setitem__("layers.0." + site, ((o != 0) | (i[0] == 0)).to(torch.uint8)))
    torch.manual_seed(1)
    x = src.double().requires_grad_(True)
    y = layer(x)
    y.backward(d_out.double())
    for site, t in masks.items():
        assert 0.8 < float(t.float().mean()) < 0.97, site
    res = TO.encoder(src, state, heads, masks=masks, p=TO.P_TRAIN, d_out=d_out)
    assert TO.rel_l2(res["out"], y.detach()) <= 1e-13
    assert TO.rel_l2(res["dsrc"], x.grad) <= 1e-12
    for k, prm in layer.named_parameters():
        assert TO.rel_l2(res["layers.0." + k], prm.grad) <= 1e-12, k


def test_attention_probability_dropout_by_formula():
    heads, src, state, _ = TO.case_inputs("odd_seq")
    S, N, E, _, F, _ = TO.CASES["odd_seq"]
    D = E // heads
    keep = TO.make_masks(state, heads, S, N, 0.3, seed=3)["layers.0.attn"]
    got = TO.encoder(src, state, heads, masks={"layers.0.attn": keep}, p=0.3)["out"]
    st = {k[len("layers.0."):]: v.double() for k, v in state.items()}
    x = src.double()
    qkv = x @ st["self_attn.in_proj_weight"].t() + st["self_attn.in_proj_bias"]
    o = torch.zeros(S, N, E, dtype=torch.float64)
    for n in range(N):
        for hd in range(heads):
            q, k, v = (qkv[:, n, i * E + hd * D: i * E + (hd + 1) * D] for i in range(3))          # (S, D): the S images at pixel n
            prob = torch.softmax(q @ k.t() / math.sqrt(D), dim=-1) * keep[n, hd].double() / 0.7
            o[:, n, hd * D:(hd + 1) * D] = prob @ v
    ln = lambda z, pre: torch.nn.functional.layer_norm(z, (E,), st[pre + ".weight"], st[pre + ".bias"], 1e-5)
    y1 = ln(x + o @ st["self_attn.out_proj.weight"].t() + st["self_attn.out_proj.bias"], "norm1")
    ff = torch.relu(y1 @ st["linear1.weight"].t() + st["linear1.bias"]) @ st["linear2.weight"].t() + st["linear2.bias"]
    assert TO.rel_l2(got, ln(y1 + ff, "norm2")) <= 1e-13


def test_parameters_are_torchs(golden):
    from sr_gan_fd_amd import model as M
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(0)
        want = torch.nn.TransformerEncoder(torch.nn.TransformerEncoderLayer(d_model=64, nhead=4), num_layers=2).state_dict()
    torch.manual_seed(0)
    m = M.TransformerEncoder(M.TransformerEncoderLayer(d_model=64, nhead=4), num_layers=2)
    got = m.state_dict()
    assert list(got) == list(want) == [str(k) for k in golden["seeded.keys"]]
    assert list(got) == ["layers.%d.%s" % (i, n) for i in range(2) for n in TO.LAYER_PARAMS]
    for k, v in want.items():
        assert torch.equal(got[k], v), k
        assert tuple(golden["seeded.shape." + k]) == tuple(v.shape), k
        assert np.abs(checksum(got[k]) - golden["seeded.sum." + k]).max() <= 1e-9, k
    assert isinstance(m, torch.nn.TransformerEncoder) and all(isinstance(l, M.TransformerEncoderLayer) for l in m.layers)
    assert m.layers[0] is not m.layers[1] and m.layers[0].linear1.out_features == 2048 and m.layers[0].dropout.p == 0.1
    assert m.compute_dtype is None and m.layers[0].compute_dtype is None
    assert "TransformerEncoderLayer" in M.__all__ and "TransformerEncoder" in M.__all__
    torch.manual_seed(0)
    lone = M.TransformerEncoderLayer(64, 4)
    assert list(lone.state_dict()) == list(TO.LAYER_PARAMS)
    assert all(torch.equal(lone.state_dict()[k], want["layers.0." + k]) for k in TO.LAYER_PARAMS)


def test_refusals(dry_run):
    from sr_gan_fd_amd import model as M
    A = dry_run
    L = M.TransformerEncoderLayer
    for kw, text in ((dict(norm_first=True), "norm_first"), (dict(activation="gelu"), "activation"), (dict(batch_first=True), "batch_first"),
                     (dict(bias=False), "bias=False")):
        with pytest.raises(A.SrganfdError, match=text):
            L(64, 4, **kw)
    with pytest.raises(A.SrganfdError, match="multiple of 32"):
        L(48, 3)
    with pytest.raises(A.SrganfdError, match="head size"):
        L(64, 8)                                                      # 8 channels a head
    with pytest.raises(A.SrganfdError, match="head size"):
        L(256, 2)                                                     # 128
    with pytest.raises(A.SrganfdError, match="dim_feedforward"):
        L(64, 4, 100)
    with pytest.raises(A.SrganfdError, match="final norm"):
        M.TransformerEncoder(L(64, 4), 2, norm=torch.nn.LayerNorm(64))
    with pytest.raises(A.SrganfdError, match="encoder_layer"):
        M.TransformerEncoder(torch.nn.TransformerEncoderLayer(64, 4), 2)
    layer, stack = L(64, 4, 96), _stack(F=96)
    x = torch.randn(3, 5, 64)
    mask = torch.zeros(3, 3)
    for kw in (dict(src_mask=mask), dict(src_key_padding_mask=torch.zeros(5, 3, dtype=torch.bool)), dict(is_causal=True)):
        with pytest.raises(A.SrganfdError, match="not supported"):
            layer(x, **kw)
    for kw in (dict(mask=mask), dict(src_key_padding_mask=torch.zeros(5, 3, dtype=torch.bool)), dict(is_causal=True)):
        with pytest.raises(A.SrganfdError, match="not supported"):
            stack(x, **kw)
    for bad in (torch.randn(3, 5, 32), torch.randn(3, 64), torch.randn(2, 3, 5, 64)):
        with pytest.raises(A.SrganfdError, match=r"expects \(S, N, 64\)"):
            layer(bad)
    with pytest.raises(A.SrganfdError, match="sequence length 129"):
        layer(torch.randn(129, 2, 64))
    A.set_dry_run(False)
    with pytest.raises(A.SrganfdError, match="not on a GPU"):
        layer(x)
    with pytest.raises(A.SrganfdError, match="not on a GPU"):
        stack(x)


def test_entry_points_refuse_bad_arguments(dry_run):
    import ctypes as C
    from sr_gan_fd_amd import ops
    A = dry_run
    L, EINVAL = A.lib(), -1
    msg = lambda: L.srganfd_last_error().decode()
    T, E = 35, 64
    t = {k: torch.zeros(T, E) for k in ("x", "r", "z", "y", "dy", "dx", "dr")}
    st, keep, gamma = torch.zeros(T), torch.ones(T, E, dtype=torch.uint8), torch.ones(E)
    ws = torch.zeros(ops.add_layernorm_workspace_bytes(T, E), dtype=torch.uint8)
    p = lambda v: None if v is None else v.data_ptr()

    def fwd(dtype=A.F32, ntok=T, e=E, eps=1e-5, **kw):
        a = {**t, "keep": keep, **kw}
        return L.srganfd_add_layernorm_fwd(dtype, p(a["x"]), p(a["r"]), p(a["keep"]), 1.0, p(gamma), p(gamma), eps, p(a["z"]), p(a["y"]), p(st), p(st), ntok, e, None)

    def bwd(dtype=A.F32, ntok=T, e=E, ws=ws, dg=gamma, db=gamma, **kw):
        a = {**t, "keep": keep, **kw}
        return L.srganfd_add_layernorm_bwd(dtype, p(a["dy"]), p(a["z"]), p(st), p(st), p(gamma), p(a["keep"]), 1.0, p(a["dx"]), p(a["dr"]), p(dg), p(db),
                                           p(ws), 0 if ws is None else ws.numel(), ntok, e, None)
    assert fwd() == 0 and fwd(keep=None) == 0 and bwd() == 0 and bwd(dg=None, db=None, ws=None) == 0
    for call in (fwd, bwd):
        for kw, text in ((dict(dtype=7), "bad dtype"), (dict(ntok=0), "ntok"), (dict(e=48), "multiple of 32"), (dict(e=4096), "multiple of 32"),
                         (dict(z=None), "null pointer"), (dict(z=t["z"].view(-1)[1:]), "aligned"), (dict(keep=keep.view(-1)[1:]), "aligned")):
            assert call(**kw) == EINVAL and text in msg(), (call.__name__, kw, msg())
    assert fwd(z=t["x"]) == EINVAL and "alias" in msg()
    assert fwd(eps=0.0) == EINVAL and "eps" in msg()
    assert bwd(dx=t["dy"]) == EINVAL and "alias" in msg()
    assert bwd(db=None) == EINVAL and "together" in msg()
    assert bwd(ws=ws[:-16]) == EINVAL and "workspace" in msg()
    assert L.srganfd_add_layernorm_workspace_bytes(T, 48) == 0
    d = lambda dtype=A.F32, x=t["x"], k=keep, y=t["y"], n=T * E: L.srganfd_dropout_apply(dtype, p(x), p(k), 2.0, p(y), n, None)
    assert d() == 0 and d(y=t["x"]) == 0
    for kw, text in ((dict(dtype=7), "bad dtype"), (dict(k=None), "null pointer"), (dict(n=12), "multiple of 8"), (dict(n=0), "multiple of 8"),
                     (dict(x=t["x"].view(-1)[1:]), "aligned")):
        assert d(**kw) == EINVAL and text in msg(), (kw, msg())
    # the short-sequence attention
    S, N, H, D = 8, 5, 4, 16
    b = dict(qkv=torch.zeros(S, N, 3 * H * D), out=torch.zeros(S, N, H * D), lse=torch.zeros(N, H, S), d_out=torch.zeros(S, N, H * D),
             d_qkv=torch.zeros(S, N, 3 * H * D), keep=torch.ones(N, H, S, S, dtype=torch.uint8))
    good = lambda **kw: ops.seq_attn_args(A.F16, S, N, H, D, **{**b, "keep_scale": 1.25, **kw})
    for entry, uses in (("fwd", ("qkv", "out", "lse")), ("bwd", ("qkv", "out", "lse", "d_out", "d_qkv"))):
        call = lambda a: getattr(L, "srganfd_seq_attention_" + entry)(C.byref(a), None)
        assert call(good()) == 0 and call(good(keep=None)) == 0
        for name in uses:
            assert call(good(**{name: None})) == EINVAL and "null pointer" in msg(), (entry, name)
        for field, value, text in (("head_dim", 8, "head_dim 8"), ("seq", 0, "non-positive"), ("seq", 129, "exceeds 128"), ("nseq", 0, "non-positive"),
                                   ("heads", 0, "non-positive"), ("dtype", 5, "bad dtype"), ("keep_scale", 0.0, "keep_scale")):
            a = good()
            setattr(a, field, value)
            assert call(a) == EINVAL and text in msg(), (entry, field, msg())
        assert call(good(qkv=b["qkv"].view(-1)[1:])) == EINVAL and "aligned" in msg()
        assert call(good(out=b["qkv"])) == EINVAL and "aliases" in msg()
    assert L.srganfd_seq_attention_bwd(C.byref(good(d_qkv=b["qkv"])), None) == EINVAL and "d_qkv aliases" in msg()
    assert L.srganfd_seq_attention_fwd(None, None) == EINVAL and "null arguments" in msg()


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


LAYER_FW = ["conv2d", "seq_attention_fwd", "conv2d", "add_layernorm_fwd", "conv2d", "dropout_apply", "conv2d", "add_layernorm_fwd"]
LAYER_BW = ["add_layernorm_bwd", "conv2d_wgrad", "conv2d", "dropout_apply", "conv2d_wgrad", "conv2d", "add_layernorm_bwd", "conv2d_wgrad", "conv2d",
            "seq_attention_bwd", "conv2d_wgrad", "conv2d"]
quiet = lambda names: [n for n in names if n != "dropout_apply"]


@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.bfloat16])
def test_module_call_sequence_at_the_consumers_shape(dry_run, dt):
    """(8, 900, 64), 4 heads, hidden 2048, two layers: the conv and weight-gradient plans take 64 -> 2048 and 2048 -> 64"""
    A = dry_run
    m = _stack()
    m.compute_dtype = dt
    rec = _Calls(A.lib())
    A._lib = rec
    try:
        x = torch.randn(8, 900, 64, requires_grad=True)
        m.train()
        out = m(x)
        assert out.shape == (8, 900, 64) and out.dtype == torch.float32
        assert rec.names == ["nchw_to_nhwc"] + 2 * LAYER_FW + ["nhwc_to_nchw"]
        masks = m.dropout_masks()
        assert sorted(masks) == sorted("layers.%d.%s" % (i, s) for i in range(2) for s in TO.SITES)
        assert masks["layers.1.attn"].shape == (900, 4, 8, 8) and masks["layers.0.dropout"].shape == (8, 900, 2048)
        assert masks["layers.0.dropout1"].shape == masks["layers.1.dropout2"].shape == (8, 900, 64) and masks["layers.0.attn"].dtype == torch.uint8
        del rec.names[:]
        out.sum().backward()
        assert rec.names == ["nchw_to_nhwc"] + 2 * LAYER_BW + ["nhwc_to_nchw"]
        assert x.grad.shape == x.shape and all(p.grad is not None and p.grad.shape == p.shape for p in m.parameters())
        del rec.names[:]
        m.eval()                                                      # no dropout launches and no masks
        out = m(x)
        out.sum().backward()
        assert rec.names == ["nchw_to_nhwc"] + 2 * quiet(LAYER_FW) + ["nhwc_to_nchw", "nchw_to_nhwc"] + 2 * quiet(LAYER_BW) + ["nhwc_to_nchw"]
        assert sorted(m.dropout_masks()) == sorted(masks)              # still those of the last training forward
        del rec.names[:]
        for p in m.parameters():                                      # frozen parameters: no weight-gradient launches
            p.requires_grad_(False)
        m(x).sum().backward()
        assert rec.names == ["nchw_to_nhwc"] + 2 * quiet(LAYER_FW) + ["nhwc_to_nchw", "nchw_to_nhwc"] + \
            [n for n in 2 * quiet(LAYER_BW) if n != "conv2d_wgrad"] + ["nhwc_to_nchw"]
        del rec.names[:]
        m(x.detach())                                                 # nothing wants a gradient: the forward alone, and no d src launch after it
        assert rec.names == ["nchw_to_nhwc"] + 2 * quiet(LAYER_FW) + ["nhwc_to_nchw"]
        del rec.names[:]
        lone = m.layers[0]
        lone.compute_dtype = dt
        lone.train()
        for p in lone.parameters():
            p.requires_grad_(True)
        lone(x.detach()).sum().backward()                             # the lone layer is a one-layer stack; no d src: its last conv is skipped
        assert rec.names == ["nchw_to_nhwc"] + LAYER_FW + ["nhwc_to_nchw", "nchw_to_nhwc"] + LAYER_BW[:-1]
    finally:
        A._lib = rec._lib


def test_second_training_forward_before_backward_raises(dry_run):
    A = dry_run
    m = _stack(F=96)
    x = torch.randn(3, 5, 64, requires_grad=True)
    first = m(x)
    m(x)
    with pytest.raises(A.SrganfdError, match="overwritten by a later forward"):
        first.sum().backward()


def test_copies_get_their_own_engine(dry_run):
    from sr_gan_fd_amd.transformer import transformer_engine
    m = _stack(F=96)
    x = torch.randn(3, 5, 64)
    assert m.dropout_masks() == {}
    m(x)
    c, q = copy.deepcopy(m), pickle.loads(pickle.dumps(m))
    assert sorted(m.dropout_masks()) == sorted("layers.%d.%s" % (i, s) for i in range(2) for s in TO.SITES) and c.dropout_masks() == {}
    assert c(x).shape == q(x).shape == (3, 5, 64)
    engines = {id(transformer_engine(t)) for t in (m, c, q)}
    assert len(engines) == 3
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), q.state_dict().values()))


def test_compute_dtype_pins_the_precision(dry_run):
    from sr_gan_fd_amd.transformer import transformer_engine
    A = dry_run
    m = _stack(F=96)
    x = torch.randn(3, 5, 64)
    m(x)
    assert transformer_engine(m)._last.dtc == A.F32
    for dt, code in ((torch.float16, A.F16), (torch.bfloat16, A.BF16)):
        m.compute_dtype = dt
        m(x)
        assert transformer_engine(m)._last.dtc == code
    m.compute_dtype = torch.float64
    with pytest.raises(A.SrganfdError, match="not supported"):
        m(x)


# ---- the conditions on the GPU cases, on the oracle alone ----
E_MAX = {"f16": 0.05, "bf16": 0.15}


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("name", list(TO.CASES))
def test_gpu_cases_are_well_conditioned(name, train):
    S, N, E, heads, F, layers = TO.CASES[name]
    if train:
        heads_, src, state, d_out = TO.case_inputs(name)
        masks = TO.make_masks(state, heads, S, N, TO.P_TRAIN, seed=9)
        for k, t in masks.items():
            assert 0.0 < float(t.float().mean()) < 1.0, k + ": the mask is not mixed"
        runs = TO.all_runs(src, state, heads, d_out, masks, TO.P_TRAIN)
    else:
        r = TO.eval_runs(name)
        src, state, d_out, masks, runs = r["src"], r["state"], r["d_out"], None, r
    for dt, emax in E_MAX.items():
        for k, ref in runs["f64"].items():
            Eg = TO.rel_l2(runs[dt][k], ref)
            assert Eg <= emax, (dt, k, Eg)
            assert TO.rel_l2(runs["f32"][k], ref) <= 1e-3, k                # 8 G stays far below what an indexing error costs (a ReLU unit that flips at its edge is in G)
    probe = {}
    TO.encoder(src, state, heads, masks=masks, p=TO.P_TRAIN if train else 0.0, probe=probe)
    for pre in TO.prefixes(state):
        prob = probe[pre + "prob"]
        assert float((prob.sum(-1) - 1).abs().max()) < 1e-12
        if S > 1:
            ent = float(-(prob * torch.log(prob.clamp_min(1e-300))).sum(-1).mean()) / math.log(S)      # mean row entropy: 0 one-hot, 1 uniform
            assert 0.1 <= ent <= 0.9, (pre, ent)
        assert float(probe[pre + "var1"].min()) > 1e3 * TO.EPS and float(probe[pre + "var2"].min()) > 1e3 * TO.EPS, pre
        live = float((probe[pre + "hidden"] > 0).double().mean())
        assert 0.2 <= live <= 0.8, (pre, live)
