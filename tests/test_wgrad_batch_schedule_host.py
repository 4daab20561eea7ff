"""CPU-only checks of the generator's backward launch list with the dense blocks' weight-gradient MFMA launches batched
(``engine._BATCH_WGRAD``, ``engine.batch_wgrads``): how the blocks group, where a batch's launch and its reduction stand, that the
stacked-gradient buffers live long enough with per-layer data gradients and with the dense-block launch, and that ``auto`` leaves a
shape whose one-block launch does not fill the chip exactly as it was.  Library dry-run mode: every launch goes through the C ABI's
checks (the batched entry point's included), no kernel runs."""
import ctypes as C

import pytest
import torch

from tests import test_launch_trace_host as T

DTYPES = [torch.float32, torch.float16]


@pytest.fixture
def dry_run():
    from sr_gan_fd_amd import _abi as A
    A.set_dry_run(True)
    try:
        yield
    finally:
        A.set_dry_run(False)


def _plan(monkeypatch, dt, num_rrdb, batch, chain="auto"):
    """(engine, plan, token) of a generator after one training-mode forward on 2x3x16x16 under the two switches"""
    from sr_gan_fd_amd import engine as E, model as M, ops
    monkeypatch.setattr(E, "_BATCH_WGRAD", batch)
    monkeypatch.setattr(ops, "DENSE_CHAIN", chain)
    torch.manual_seed(0)
    g = M.bsrgan_x4(num_rrdb=num_rrdb)
    g.compute_dtype = dt
    eng = E.generator_engine(g)
    eng.forward(torch.rand(2, 3, 16, 16), True)
    return g, eng, eng._last, eng.token


def _sig(it):
    """what an item is and launches, without the addresses of per-plan buffers"""
    out = [it.kind]
    for name in ("args", "jobs", "arr"):
        v = getattr(it, name, None)
        if isinstance(v, (C.Structure, C.Array)):
            out.append(bytes(memoryview(v).cast("B")) if not isinstance(v, C.Structure) else bytes(v))
    for name in ("lo", "hi", "n", "slot", "dw_off", "block", "label", "name", "op"):
        if hasattr(it, name):
            out.append((name, getattr(it, name)))
    return out


@pytest.mark.parametrize("chain", ["0", "1"])
@pytest.mark.parametrize("num_rrdb,groups", [(2, [3, 3]), (3, [4, 1, 4])])
@pytest.mark.parametrize("dt", DTYPES)
def test_forced_on_groups_the_blocks_and_reduces_each_batch_at_once(dry_run, monkeypatch, dt, num_rrdb, groups, chain):
    from sr_gan_fd_amd import engine as E, ops
    g, eng, sp, token = _plan(monkeypatch, dt, num_rrdb, "1", chain)
    kinds = [it.kind for it in sp.bw]
    chained = "chain" in kinds
    assert chained == (chain == "1" and dt != torch.float32)            # the dense-block launch is a 16-bit kernel
    assert len(sp.dy) == (E._BATCH_REDUCE + 1 if chained else 4)
    batches = [it for it in sp.bw if it.kind == "wgrad_partial_batch"]
    assert [b.n for b in batches] == groups
    assert "wgrad_partial" not in kinds and not any(it.kind == "wgrad" and it.block is not None for it in sp.bw)
    # the blocks, last to first, each once; a batch's plans share the pixel splits: 1 / n of one block's (4 tiles here), at least 1
    assert [p.block for b in batches for p in b.partials] == list(range(eng.R - 1, -1, -1))
    for b in batches:
        assert {p.plan.splits for p in b.partials} == {max(1, 4 // b.n)}
        assert len({p.ws.data_ptr() for p in b.partials}) == b.n
    # every batch is followed by the reduction of exactly its partials
    for i, it in enumerate(sp.bw):
        if it.kind == "wgrad_partial_batch":
            nxt = sp.bw[i + 1]
            assert nxt.kind == "wgrad_reduce" and nxt.partials == it.partials
            assert [j.workspace for j in nxt.jobs] == [j.workspace for j in it.jobs]
    assert kinds.count("wgrad_reduce") == len(groups)
    # the buckets are those of the unbatched list
    ranges = [(it.lo, it.hi) for it in sp.bw if it.kind == "ready"]
    _, _, sp0, _ = _plan(monkeypatch, dt, num_rrdb, "0", chain)
    assert ranges == [(it.lo, it.hi) for it in sp0.bw if it.kind == "ready"] and len(ranges) == 3
    # and the list runs through the library's checks (dry run: the batched entry point validates every job)
    eng.backward(sp, token, torch.rand(2, 3, 64, 64), True, False)


@pytest.mark.parametrize("chain", ["0", "1"])
def test_lifetime_check_refuses_a_buffer_overwritten_before_the_batch_reads_it(dry_run, monkeypatch, chain):
    """the check in batch_wgrads is what proves the rotation: with the dense-block launch and only four stacked-gradient buffers, a
    batch of four reads a buffer that the last block's launch has overwritten"""
    from sr_gan_fd_amd import _abi as A, engine as E, ops
    g, eng, sp, _ = _plan(monkeypatch, torch.float16, 3, "0", chain)
    slots = sp.wg_ws4
    plain = []                                                   # the list before batch_reductions: partials back to Wgrad items
    for it in sp.bw:
        if it.kind == "wgrad_partial":
            plain.append(ops.Wgrad(it.plan, it.x, it.dy, dw_off=it.dw_off, block=it.block))
        elif it.kind != "wgrad_reduce":
            plain.append(it)
    assert len(sp.dy) == 4
    if chain == "1":
        with pytest.raises(A.SrganfdError, match="overwritten"):
            E.batch_wgrads(plain, slots, lambda wg, n: wg.plan)
    else:
        out = E.batch_wgrads(plain, slots, lambda wg, n: wg.plan)
        assert [it.n for it in out if it.kind == "wgrad_partial_batch"] == [4, 1, 4]


@pytest.mark.parametrize("dt", DTYPES)
def test_auto_leaves_a_small_shape_as_it_was(dry_run, monkeypatch, dt):
    """2x3x16x16 has 4 pixel tiles per block against 36 splits: a one-block launch does not fill the chip, ``auto`` does not batch"""
    _, _, sp_auto, _ = _plan(monkeypatch, dt, 2, "auto")
    _, _, sp_off, _ = _plan(monkeypatch, dt, 2, "0")
    assert not sp_auto.batch_wgrad and len(sp_auto.dy) == len(sp_off.dy) == 4
    assert len(sp_auto.bw) == len(sp_off.bw)
    for a, b in zip(sp_auto.bw, sp_off.bw):
        assert _sig(a)[0] == _sig(b)[0] and [x for x in _sig(a) if isinstance(x, tuple)] == [x for x in _sig(b) if isinstance(x, tuple)]


@pytest.mark.parametrize("dt", DTYPES)
def test_auto_launches_what_off_launches(dry_run, monkeypatch, dt):
    """... and the two lists make the same library calls, argument for argument (pointers as the launch trace records them)"""
    from sr_gan_fd_amd import _abi as A
    traces = []
    for mode in ("auto", "0"):
        g, eng, sp, token = _plan(monkeypatch, dt, 2, mode)
        rec = T.Recorder(A.lib())
        A._lib = rec
        try:
            eng.backward(sp, token, torch.ones(2, 3, 64, 64), True, False)
        finally:
            A._lib = rec._lib
        traces.append(rec.launches)
    assert traces[0] == traces[1] and not any(c[0] == "srganfd_conv2d_wgrad_partial_batch" for c in traces[0])


def test_batched_entry_point_refuses_bad_batches(dry_run):
    """njobs out of range, a null pointer, other geometry, other splits, another view form and a short workspace: EINVAL with a message"""
    from sr_gan_fd_amd import _abi as A, ops
    L = A.lib()
    convs = [dict(cin=64, cout=64, dw_off=0, db_off=64 * 64 * 9, co_dst=64, ci_dst=64)]
    mk = lambda h=16, splits=2, alpha=1.0: ops.WgradPlan("cpu", A.F16, 2, h, 16, 64, 64, [dict(convs[0], alpha=alpha)], splits=splits)
    p, p_alpha, p_geo, p_split = mk(), mk(alpha=0.2), mk(h=24), mk(splits=3)
    x, dy = torch.zeros(2, 24, 16, 64, dtype=torch.float16), torch.zeros(2, 24, 16, 64, dtype=torch.float16)
    ws = torch.zeros(max(q.workspace_bytes for q in (p, p_geo, p_split)), dtype=torch.uint8)

    def call(plans, n=None, xs=None, wbytes=None, null=False):
        jobs = (A.WgradPartialJob * max(1, len(plans)))()
        for j, q in zip(jobs, plans):
            j.plan_host, j.plan_dev, j.x, j.dy = C.addressof(q.host), q.dev.data_ptr(), A.view(x), A.view(dy)
            j.workspace, j.workspace_bytes = ws.data_ptr(), ws.numel() if wbytes is None else wbytes
        if xs is not None:
            jobs[len(plans) - 1].x = xs
        if null:
            jobs[len(plans) - 1].dy = A.NULL_VIEW
        return L.srganfd_conv2d_wgrad_partial_batch(jobs, len(plans) if n is None else n, None)
    assert call([p]) == 0 and call([p, p_alpha]) == 0 and call([p] * 8) == 0          # task tables may differ
    bad = ((lambda: call([p], n=0), "jobs"), (lambda: call([p] * 8, n=9), "jobs"), (lambda: call([p, p], null=True), "null"),
           (lambda: call([p, p_geo]), "geometry"), (lambda: call([p, p_split]), "geometry"),
           (lambda: call([p, p], xs=A.view(x, c0=32)), "views"), (lambda: call([p, p], xs=A.view(x, planar=1)), "views"),
           (lambda: call([p, p], wbytes=p.workspace_bytes - 4), "workspace"))
    for fn, word in bad:
        rc = fn()
        assert rc != 0 and word in L.srganfd_last_error().decode(), (rc, word, L.srganfd_last_error().decode())
        with pytest.raises(A.SrganfdError):
            A.check(rc, "conv2d_wgrad_partial_batch")
