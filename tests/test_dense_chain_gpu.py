"""LDS-resident dense-block launch (csrc/dense_chain.hip, srganfd_dense_chain; 16 x 16-, 12 x 16- or 8 x 16-pixel tiles, one per CU and pass) against the separate srganfd_conv2d launches it replaces:
the five convs of _ResidualDenseBlock.forward (BSRGAN/model.py:51-62: four growth convs with bias + LeakyReLU written into the block's
own buffer, the closing 192 -> 64 conv with the residual epilogue) and the five launches of its data-gradient pass (masks from the saved
activations, residual adds on the closing launch), at the reference's crop sizes and at ragged ones, NHWC and planar buffers, several
images per pass and several passes per call.  Same accumulation order and epilogue formula -> the comparison bound is one rounding of
the stored 16-bit value (and the CPU oracle comparison of the whole generator runs through the engine in test_generator_gpu.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _views(buf, planar):
    from sr_gan_fd_amd import _abi as A
    return lambda c0=0: A.view(buf, c0=c0, planar=planar)


def _build(dtype, n, h, w, planar, backward, seed=0):
    """the five launches of a dense block over fresh buffers; returns (args list, buffers to compare, keep-alive list)"""
    from sr_gan_fd_amd import _abi as A, ops
    torch.manual_seed(seed)
    dt = ops.DT[dtype]
    Cc, G = 64, 32
    buf = torch.zeros(n, h, w, 192, device="cuda", dtype=dtype)
    x0 = (torch.randn(n, h, w, Cc, device="cuda") * 0.6).to(dtype)
    if planar:
        buf.view(n, 6, h, w, 32)[:, :2].copy_(x0.view(n, h, w, 2, 32).permute(0, 3, 1, 2, 4))
    else:
        buf[..., :Cc].copy_(x0)
    out = torch.full((n, h, w, Cc), 7.0, device="cuda", dtype=dtype)
    V, VO = _views(buf, planar), _views(out, 0)
    keep, args = [buf, out], []
    r1 = (torch.randn(n, h, w, Cc, device="cuda")).to(dtype)
    r2 = (torch.randn(n, h, w, Cc, device="cuda")).to(dtype)
    act = (torch.randn(n, h, w, 192, device="cuda")).to(dtype)           # "saved activations": the sign gives the LeakyReLU' mask
    keep += [r1, r2, act]
    for k in range(5):
        cin, cout = Cc + k * G, (Cc if k == 4 else G)
        wt = torch.randn(cout, cin, 3, 3, device="cuda") / (3.0 * cin ** 0.5)
        wp = ops.pack_single(wt, dt)
        b = torch.randn(cout, device="cuda") * 0.1
        keep += [wp, b]
        if k < 4:
            kw = dict(mask=A.view(act, c0=Cc + (3 - k) * G), mask_slope=0.2) if backward else dict(bias=b, act=A.ACT_LRELU, slope=0.2)
            args.append(ops.conv_args(dt, V(), V(cin), wp, n, h, w, cin, cout, **kw))
        else:
            kw = dict(r1=A.view(r1), r1_scale=0.2, r2=A.view(r2), r2_scale=1.0) if backward else \
                dict(bias=b, post_scale=0.04, r1=V(), r1_scale=0.2, r2=A.view(r2), r2_scale=1.0)
            args.append(ops.conv_args(dt, V(), VO(), wp, n, h, w, cin, cout, **kw))
    return args, (buf, out), keep


@pytest.mark.parametrize("rows", [None, 12, 16], ids=["tile-rows-auto", "tile-rows-12", "tile-rows-16"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("backward", [False, True], ids=["forward", "data-gradient"])
@pytest.mark.parametrize("shape", [(2, 16, 32, 1), (3, 21, 45, 1), (16, 32, 32, 1), (8, 60, 60, 1), (16, 72, 72, 1), (2, 24, 40, 0), (1, 8, 8, 1)],
                         ids=lambda s: "n%d_%dx%d_%s" % (s[0], s[1], s[2], "planar" if s[3] else "nhwc"))
def test_dense_chain_equals_the_separate_launches(dtype, backward, shape, rows, monkeypatch):
    """(the library picks 8 x 16 tiles when the batch is one pass that way -- every shape here but 16 x 72 x 72 --, else 12 x 16, else
    16 x 16; ``rows`` forces one form everywhere through the A/B switch SRGANFD_DC_RPW)"""
    from sr_gan_fd_amd import ops
    if rows is not None:
        monkeypatch.setenv("SRGANFD_DC_RPW", str(rows // 4))
    n, h, w, planar = shape
    a_ref, (buf_ref, out_ref), k1 = _build(dtype, n, h, w, planar, backward)
    a_dc, (buf_dc, out_dc), k2 = _build(dtype, n, h, w, planar, backward)
    assert torch.equal(buf_ref, buf_dc)
    for a in a_ref:
        ops.conv2d(a)
    chain = ops.DenseChain(a_dc, buf_dc.device)
    assert chain.ok
    chain.run()
    torch.cuda.synchronize()
    assert chain.errors() == 0
    scale = buf_ref.float().abs().max().item()
    e_buf = (buf_ref.float() - buf_dc.float()).abs().max().item() / scale
    e_out = (out_ref.float() - out_dc.float()).abs().max().item() / (out_ref.float().abs().max().item() + 1e-30)
    same = torch.equal(buf_ref, buf_dc) and torch.equal(out_ref, out_dc)
    print(f"dense chain {dtype} n{n} {h}x{w}: buffer err {e_buf:.2e}, output err {e_out:.2e}, bitwise {same}")
    # one rounding of a stored 16-bit value can differ where an fp32 sum lands on a rounding boundary (the epilogue is an explicit fma chain
    # here, mul + add where the compiler chose so in conv_igemm) and propagates through the later layers
    tol = 4e-3 if dtype == torch.float16 else 3e-2
    assert torch.isfinite(out_dc.float()).all() and e_buf < tol and e_out < tol
    # a second run over the same buffers (flags are epoch-valued: the launch before advanced the epoch) gives the same bits: the launch is deterministic
    snap_b, snap_o = buf_dc.clone(), out_dc.clone()
    chain.run()
    torch.cuda.synchronize()
    assert chain.errors() == 0 and torch.equal(snap_b, buf_dc) and torch.equal(snap_o, out_dc)


def test_dense_chain_refuses_what_it_cannot_run():
    from sr_gan_fd_amd import _abi as A, ops
    args, _, keep = _build(torch.float16, 1, 16, 32, 1, False)
    assert ops.DenseChain(args, "cuda").ok
    assert not ops.DenseChain(args[:1], "cuda").ok                       # fewer than two layers
    assert not ops.DenseChain(args[1:], "cuda").ok                       # does not start at the 64-channel layer
    big, _, keep2 = _build(torch.float16, 1, 8 * 40, 32 * 8, 1, False)   # 320 tiles of one image: more than the device has CUs
    assert not ops.DenseChain(big, "cuda").ok
    # "auto": batches that fit one pass of 16 x 16 tiles on the 256 CUs
    assert not ops.dense_chain_wanted(32, 128, 128) and not ops.dense_chain_wanted(16, 72, 72) and ops.dense_chain_wanted(16, 32, 32) and ops.dense_chain_wanted(8, 60, 60)


def test_dense_chain_beside_kernels_of_another_stream():
    """The launch needs one workgroup per CU resident at once; kernels of another stream (in training: RCCL's all-reduce, the side-stream
    weight gradients) may hold CUs for a while.  The chain then waits for them (its workgroups poll their neighbours' flags) and must give the
    same bits, with no hand-off wait given up."""
    from sr_gan_fd_amd import ops
    n, h, w = 16, 32, 32
    a_ref, (buf_ref, out_ref), k1 = _build(torch.float16, n, h, w, 1, False)
    a_dc, (buf_dc, out_dc), k2 = _build(torch.float16, n, h, w, 1, False)
    for a in a_ref:
        ops.conv2d(a)
    chain = ops.DenseChain(a_dc, buf_dc.device)
    assert chain.ok
    chain.run()
    torch.cuda.synchronize()
    want_b, want_o = buf_dc.clone(), out_dc.clone()
    side = torch.cuda.Stream()
    big_a = torch.randn(4096, 4096, device="cuda", dtype=torch.float16)
    big_b = torch.randn(4096, 4096, device="cuda", dtype=torch.float16)
    for rep in range(5):
        buf_dc.view(n, 6, h, w, 32)[:, 2:].zero_(); out_dc.fill_(7.0)      # planar groups 2..5 = the growth layers' outputs
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(6):
                big_c = big_a @ big_b             # chip-filling GEMMs with LDS of their own
        for _ in range(4):
            chain.run()
        torch.cuda.synchronize()
        assert chain.errors() == 0
        assert torch.equal(buf_dc, want_b) and torch.equal(out_dc, want_o)


@pytest.mark.parametrize("batch,size,num_rrdb,rows", [
    (16, 32, 23, 8),      # ESRGAN/esrgan_config.py:73-74, the whole 23-RRDB generator: 128 tiles of 8 x 16
    (16, 48, 4, 12),      # ESRGAN/rrdbnet_config.py:51-52: 192 tiles of 12 x 16
    (4, 128, 2, 16),      # batch 4 at the headline crop: 256 tiles of 16 x 16
])
def test_generator_iteration_at_the_reference_crops_through_the_launch_meets_the_tolerance(batch, size, num_rrdb, rows):
    """A generator-only training iteration (train_rrdbnet.py:244-267) in float16 -- the scripts' autocast dtype -- at the crop sizes the
    reference's configs ship, where the engine takes the dense-block launch for every dense block, forward and data gradient: SR and
    loss against the fp32 CPU oracle within BASELINE.json's 1e-3 (SR absolute, loss relative), the Adam update against the oracle's as one
    relative L2 norm (< 2e-2: f16 gradients; measured 1.3e-3 ... 7.1e-3), and the same iteration with the per-layer launches (SRGANFD_DENSE_CHAIN=0) within one
    16-bit rounding's propagation of it (SR 2e-4; measured: identical bits, SR max error against the oracle 6.0e-4 at 23 RRDB)."""
    from oracle import srgan_oracle as O
    from sr_gan_fd_amd import model as M, ops
    from sr_gan_fd_amd.trainer import GeneratorTrainer
    from tests.util import scaled_init
    torch.manual_seed(5)
    lr_img, gt = torch.rand(batch, 3, size, size), torch.rand(batch, 3, 4 * size, 4 * size)

    def gen():
        torch.manual_seed(0)
        g = M.bsrgan_x4(num_rrdb=num_rrdb)
        scaled_init(g, 3.0, 0.5)
        return g
    g0 = gen()
    G = {k: v.detach().clone() for k, v in g0.state_dict().items()}
    G0 = {k: v.clone() for k, v in G.items()}
    opt = O.AdamState(G, O.g_param_names(G))
    want_loss, want_sr = O.g_only_step(G, opt, lr_img, gt, upscale=4, lr=1e-4, betas=(0.9, 0.99), eps=1e-4)
    res = {}
    old = ops.DENSE_CHAIN
    try:
        for mode in ("auto", "0"):
            ops.DENSE_CHAIN = mode
            g = gen()
            g.compute_dtype = torch.float16
            tr = GeneratorTrainer(g.cuda().train(), lr=1e-4, betas=(0.9, 0.99), eps=1e-4, ema_decay=0.999)
            loss = tr.step(lr_img.cuda(), gt.cuda())
            torch.cuda.synchronize()
            sp = tr.eng._last
            chains = [it for it in sp.fw + sp.bw if it.kind == "chain"]
            assert len(chains) == (6 * num_rrdb if mode == "auto" else 0), (mode, len(chains))
            if mode == "auto":
                assert ops.dense_chain_giveups(torch.device("cuda", torch.cuda.current_device())) == 0
            res[mode] = (loss.item(), tr.sr.float().cpu(), {k: v.detach().float().cpu() for k, v in g.state_dict().items()})
    finally:
        ops.DENSE_CHAIN = old
    loss, sr, sd = res["auto"]
    err_sr = (sr - want_sr).abs().max().item()
    num = sum(((sd[k] - G[k]) ** 2).sum().item() for k in G)
    den = sum(((G[k] - G0[k]) ** 2).sum().item() for k in G)
    err_w = (num / den) ** 0.5
    d_sr = (sr - res["0"][1]).abs().max().item()
    print(f"batch {batch} {size}->{4 * size}, {num_rrdb} RRDB, {rows} x 16 tiles: loss {loss:.6f} (oracle {want_loss:.6f}), SR max err {err_sr:.2e}, "
          f"Adam-update rel L2 err {err_w:.2e}; per-layer launches: loss {res['0'][0]:.6f}, SR diff {d_sr:.2e}")
    assert abs(loss - want_loss) < 1e-3 * abs(want_loss) and err_sr < 1e-3 and err_w < 2e-2
    assert d_sr < 2e-4 and abs(loss - res["0"][0]) < 1e-4 * abs(want_loss)


# ---- every epilogue kind against the float64 formula, layer by layer ----
# dense_chain.hip promises conv_igemm.hip's arithmetic contract, so each layer of a chain is held to the bound tests/test_conv_paths_gpu.py
# holds conv_igemm to (conv_oracle.bound, unchanged): layer k's stored output against conv_oracle.conv2d over the chain's OWN stored
# channels [0, 64 + 32 k), so no error carries from layer to layer.  n = 2 images of 35 x 37 pixels: ragged both ways, at least 3 x 3
# tiles in every tile form (a tile with all eight neighbours, every border kind), one pass.
# SRGANFD_DC_KINDS_REPORT=<file> appends the worst err / bound per epilogue kind and dtype (profiles/dense_chain_kinds_fp64.txt).
KN, KH, KW = 2, 35, 37
_FWD = dict(bias=True, act=1, slope=0.2, alpha=1.0, alpha_dev=None, post_scale=1.0, ops="none")       # act: conv_oracle.ACT_*
_OPS = {"none": 0, "mask": 1, "r1": 2, "r1r2": 3}


def _L(**kw):
    return dict(_FWD, **kw)


# name -> layers (the last one closes the chain: 64 channels into its own buffer; the others grow the block buffer by 32 channels)
KIND_CHAINS = {
    # the eight growth kinds: operands none / mask / r1 / r1 + r2, max form (LeakyReLU 0.2, post_scale 1) and select form
    "grow_max": [_L(alpha=1.5), _L(ops="mask"), _L(ops="r1", bias=False), _L(ops="r1r2", alpha_dev=0.6), _L(act=0, post_scale=0.04, ops="r1r2")],
    "grow_select": [_L(post_scale=-0.5), _L(slope=1.5, ops="mask", alpha=0.75), _L(post_scale=-0.5, ops="r1", bias=False), _L(slope=1.5, ops="r1r2"),
                    _L(act=0, post_scale=-0.5, ops="mask", alpha_dev=1.75)],
    # the eight closing kinds behind 1, 2 and 3 growth layers
    "close2_max_none": [_L(alpha=1.25), _L(act=2, post_scale=0.5)],
    "close3_max_mask": [_L(), _L(alpha=0.75, bias=False), _L(act=0, bias=False, ops="mask")],
    "close4_max_r1": [_L(), _L(ops="mask"), _L(alpha=1.5), _L(act=0, post_scale=0.04, ops="r1", alpha=2.0)],
    "close2_max_r1r2": [_L(alpha_dev=0.7), _L(act=0, post_scale=0.04, ops="r1r2", alpha=0.5)],
    "close3_select_none": [_L(), _L(alpha=1.5), _L(act=1, slope=1.5, alpha=0.75)],
    "close4_select_mask": [_L(alpha=0.5), _L(), _L(ops="r1"), _L(act=0, post_scale=-0.5, bias=False, ops="mask")],
    "close2_select_r1": [_L(alpha=1.5, alpha_dev=1.25), _L(act=1, post_scale=-0.5, ops="r1")],
    "close3_select_r1r2": [_L(), _L(alpha=0.75), _L(act=1, slope=1.5, ops="r1r2", alpha=1.25)],
}


def epilogue_kind(layer, last):
    """dense_chain_fill's formula: 4 (growth layer) + operands (3 r1 + r2, 2 r1, 1 mask, 0 none) + 8 (activation in max form)"""
    neg = layer["slope"] if layer["act"] == 1 else (0.0 if layer["act"] == 2 else 1.0)
    ps_pos, ps_neg = layer["post_scale"], neg * layer["post_scale"]
    return 4 * (not last) + _OPS[layer["ops"]] + 8 * (ps_neg >= 0 and ps_pos >= ps_neg)


def test_kind_chains_cover_every_epilogue_kind():
    kinds = {epilogue_kind(l, i == len(ls) - 1) for ls in KIND_CHAINS.values() for i, l in enumerate(ls)}
    assert kinds == set(range(16)), sorted(kinds)
    assert {epilogue_kind(l, False) for l in KIND_CHAINS["grow_max"][:4]} == {12, 13, 14, 15}
    assert {epilogue_kind(l, False) for l in KIND_CHAINS["grow_select"][:4]} == {4, 5, 6, 7}
    closing = [ls for nm, ls in KIND_CHAINS.items() if nm.startswith("close")]
    assert sorted(epilogue_kind(ls[-1], True) for ls in closing) == [0, 1, 2, 3, 8, 9, 10, 11]
    assert all(sum(len(ls) == k for ls in closing) >= 2 for k in (2, 3, 4))
    assert all(any(l["alpha"] != 1.0 for l in ls) for ls in KIND_CHAINS.values())
    assert sum(any(l["alpha_dev"] for l in ls) for ls in KIND_CHAINS.values()) >= 2
    assert any(not l["bias"] for ls in KIND_CHAINS.values() for l in ls[:-1])


KIND_RATIOS = {}       # (epilogue kind, dtype) -> worst err / bound seen


@pytest.fixture(scope="module")
def kinds_report():
    import os
    yield
    lines = ["%8.4f  kind %2d  %s" % (r, k, dt) for (k, dt), r in sorted(KIND_RATIOS.items())]
    print("\nworst err / bound per epilogue kind\n" + "\n".join(lines))
    path = os.environ.get("SRGANFD_DC_KINDS_REPORT")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


_KIND_DATA = {}        # (chain, dtype) -> host data, made once for the three tile forms and both layouts


def _kind_data(name, dtype):
    from tests.test_conv_paths_gpu import f32r
    key = (name, dtype)
    if key not in _KIND_DATA:
        _KIND_DATA.clear()
        g = torch.Generator().manual_seed(4321 + 7 * len(name) + sorted(KIND_CHAINS).index(name))
        rnd = lambda *s: torch.randn(*s, generator=g)
        D = dict(x0=(rnd(KN, KH, KW, 64) * 0.6).to(dtype), layers=[])
        for k, l in enumerate(KIND_CHAINS[name]):
            last = k == len(KIND_CHAINS[name]) - 1
            cin, cout = 64 + 32 * k, (64 if last else 32)
            d = dict(wt=rnd(cout, cin, 3, 3) / (3.0 * cin ** 0.5), bias=rnd(cout) * 0.1 if l["bias"] else None,
                     alpha_dev=torch.tensor([l["alpha_dev"]], dtype=torch.float32) if l["alpha_dev"] else None)
            for nm in {"none": (), "mask": ("mask",), "r1": ("r1",), "r1r2": ("r1", "r2")}[l["ops"]]:
                d[nm] = rnd(KN, KH, KW, cout).to(dtype)
            d["scalars"] = dict(act=l["act"], slope=f32r(l["slope"]), alpha=f32r(l["alpha"]), post_scale=f32r(l["post_scale"]),
                                r1_scale=f32r(0.2 if "r1" in d else 0.0), r2_scale=f32r(-1.0 if "r2" in d else 0.0), mask_slope=f32r(0.25))
            D["layers"].append(d)
        _KIND_DATA[key] = D
    return _KIND_DATA[key]


@pytest.mark.parametrize("rows", [8, 12, 16], ids=lambda r: "tile-rows-%d" % r)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("name", list(KIND_CHAINS))
def test_every_epilogue_kind_layer_by_layer_against_fp64(name, dtype, rows, monkeypatch, kinds_report):
    from sr_gan_fd_amd import _abi as A, ops
    from tests import conv_oracle as O
    monkeypatch.setenv("SRGANFD_DC_RPW", str(rows // 4))
    dt, layers, D = ops.DT[dtype], KIND_CHAINS[name], _kind_data(name, dtype)
    nl = len(layers)
    for planar in (0, 1):
        what = f"{name} {dtype} {rows} x 16 tiles {'planar' if planar else 'nhwc'}"
        g = torch.Generator().manual_seed(99)
        blk = O.Buf(KN, KH, KW, 192, dtype, planar)
        blk.put(0, D["x0"])
        blk.upload()
        out = O.Buf(KN, KH, KW, 128, dtype, planar).upload()             # the closing layer writes channels [32, 96)
        keep, args = [], []
        for k, (l, d) in enumerate(zip(layers, D["layers"])):
            last = k == nl - 1
            cin, cout = 64 + 32 * k, (64 if last else 32)
            wp = ops.pack_single(d["wt"].cuda(), dt)
            kw = dict(d["scalars"], bias=d["bias"].cuda() if d["bias"] is not None else None, alpha_dev=d["alpha_dev"].cuda() if d["alpha_dev"] is not None else None)
            for j, nm in enumerate(("r1", "r2", "mask")):
                if nm in d:        # a slice at a non-zero multiple-of-32 offset of a wider tensor of other values
                    b = O.Buf(KN, KH, KW, 128, dtype, planar, fill="garbage", gen=g)
                    c0 = 32 if last else 32 * (1 + (k + j) % 3)
                    b.put(c0, d[nm])
                    kw[nm] = b.upload().view(A, c0)
                    keep.append(b)
            keep += [wp, kw["bias"], kw["alpha_dev"]]
            args.append(ops.conv_args(dt, blk.view(A), out.view(A, 32) if last else blk.view(A, cin), wp, KN, KH, KW, cin, cout, **kw))
        chain = ops.DenseChain(args, "cuda")
        assert chain.ok, what
        chain.run()
        torch.cuda.synchronize()
        assert chain.errors() == 0, what
        got_blk, got_out = blk.download(), out.download()
        blk.assert_outside_untouched(got_blk, 64, 32 * (nl - 1), what + " block buffer")
        out.assert_outside_untouched(got_out, 32, 64, what + " closing output")
        for k, (l, d) in enumerate(zip(layers, D["layers"])):
            last = k == nl - 1
            cin, cout = 64 + 32 * k, (64 if last else 32)
            ref, _, mag = O.conv2d(got_blk[..., :cin], d["wt"].to(dtype), bias=d["bias"], alpha_dev=d["alpha_dev"], r1=d.get("r1"), r2=d.get("r2"),
                                   mask=d.get("mask"), **d["scalars"])
            got = got_out[..., 32:96] if last else got_blk[..., cin:cin + 32]
            ratio, at = O.worst_ratio(got, ref, mag, 9 * cin, dtype)
            kind = epilogue_kind(l, last)
            print(f"{what} layer {k} kind {kind}: worst err / bound {ratio:.4f}")
            KIND_RATIOS[(kind, str(dtype))] = max(KIND_RATIOS.get((kind, str(dtype)), 0.0), ratio)
            assert ratio <= 1.0, f"{what} layer {k} (kind {kind}): element {at} is {ratio:.3f} times its bound"
