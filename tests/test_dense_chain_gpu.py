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
    # a second run over the same buffers (flags re-zeroed on the stream) gives the same bits: the launch is deterministic
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
