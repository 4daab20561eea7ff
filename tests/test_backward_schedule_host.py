"""CPU-only checks of the generator's backward launch list (engine.TrunkEngine._plan_backward) for a six-block trunk
(``bsrgan_x4(num_rrdb=2)``; the reductions for a nine-block one too): where the dense blocks' weight-gradient slabs are reduced -- one batched reduction per at most
``engine._BATCH_REDUCE`` blocks, each block's slabs in a workspace slot of their own, reduced before anything that reads the flat
gradient's range or shares workspace slot 0 -- and where the gradient buckets of the data-parallel exchange are announced.  Library
dry-run mode: every launch goes through the C ABI's checks, no kernel runs."""
import pytest
import torch

from tests import test_launch_trace_host as T

DTYPES = [torch.float32, torch.float16]


def _trained_plan(dt, num_rrdb=2):
    """a generator after one training-mode forward on 2x3x16x16: (module, engine, plan, token)"""
    from sr_gan_fd_amd import engine as E, model as M
    torch.manual_seed(0)
    g = M.bsrgan_x4(num_rrdb=num_rrdb)
    g.compute_dtype = dt
    eng = E.generator_engine(g)
    eng.forward(torch.rand(2, 3, 16, 16), True)
    return g, eng, eng._last, eng.token


@pytest.fixture
def dry_run():
    from sr_gan_fd_amd import _abi as A
    A.set_dry_run(True)
    try:
        yield
    finally:
        A.set_dry_run(False)


# six blocks: the bucket marker behind block 3 (R // 2) parts them three and three; nine blocks: blocks 8..5 fill a batch, block 4 is
# reduced alone before the marker, blocks 3..0 fill a batch
@pytest.mark.parametrize("num_rrdb,batches", [(2, [3, 3]), (3, [4, 1, 4])])
@pytest.mark.parametrize("dt", DTYPES)
def test_slab_reductions_are_scheduled_in_the_plan(dry_run, dt, num_rrdb, batches):
    from sr_gan_fd_amd import engine as E
    g, eng, sp, _ = _trained_plan(dt, num_rrdb)
    assert E._BATCH_REDUCE == 4 and eng.R == 3 * num_rrdb
    partials = [it for it in sp.bw if it.kind == "wgrad_partial"]
    reduces = [it for it in sp.bw if it.kind == "wgrad_reduce"]
    assert len(partials) == eng.R and [r.n for r in reduces] == batches
    assert not any(it.kind == "wgrad" and it.block is not None for it in sp.bw)
    pending = []                       # partials not yet covered by a reduce item
    for it in sp.bw:
        if it.kind == "wgrad_partial":
            pending.append(it)
        elif it.kind == "wgrad_reduce":
            # no more than a batch, in slots (and workspaces) of their own, and exactly the partials since the last reduction
            assert 1 <= it.n <= E._BATCH_REDUCE
            assert it.partials == pending
            assert len({p.slot for p in pending}) == it.n and len({p.ws.data_ptr() for p in pending}) == it.n
            assert [j.workspace for j in it.jobs] == [p.ws.data_ptr() for p in pending]
            pending = []
        elif it.kind in ("ready", "wgrad") or (it.kind == "thin" and it.is_wgrad):
            # a bucket is announced, or a launch shares workspace slot 0: nothing may be waiting for its reduction
            assert not pending, it.kind
    assert not pending
    # the buckets are disjoint and cover the flat gradient
    ranges = sorted((it.lo, it.hi) for it in sp.bw if it.kind == "ready")
    assert len(ranges) == 3 and ranges[0][0] == 0 and ranges[-1][1] == eng.fp.total
    assert all(a[1] == b[0] and a[0] < a[1] for a, b in zip(ranges, ranges[1:] + [(eng.fp.total, 0)]))


@pytest.mark.parametrize("dt", DTYPES)
def test_without_batched_reduction_the_blocks_keep_plain_weight_gradients(dry_run, monkeypatch, dt):
    from sr_gan_fd_amd import engine as E
    monkeypatch.setattr(E, "_BATCH_REDUCE", 1)
    g, eng, sp, _ = _trained_plan(dt)
    assert not any(it.kind in ("wgrad_partial", "wgrad_reduce") for it in sp.bw)
    assert sorted(it.block for it in sp.bw if it.kind == "wgrad" and it.block is not None) == list(range(6))


# (library calls enqueued by backward() so far, lo, hi) at each on_ready call, recorded from the commit before the schedule moved
# into the plan (c777a55), where backward() decided the reductions while launching: the buckets are announced at the same points
# of the launch sequence.  lo / hi are elements of the flat gradient.
ON_READY_PARENT = {
    torch.float32: [(14, 1440640, 1590084), (32, 721216, 1440640), (54, 0, 721216)],
    torch.float16: [(11, 1440640, 1590084), (18, 721216, 1440640), (27, 0, 721216)],
}


def _on_ready_notes(dt):
    from sr_gan_fd_amd import _abi as A
    g, eng, sp, token = _trained_plan(dt)
    rec = T.Recorder(A.lib())
    notes = []

    def on_ready(flat_grad, lo, hi):
        assert flat_grad.numel() == eng.fp.total
        notes.append((len(rec.launches), lo, hi))
    A._lib = rec
    try:
        eng.backward(sp, token, torch.rand(2, 3, 64, 64), True, False, on_ready=on_ready)
    finally:
        A._lib = rec._lib
    return notes, len(rec.launches)


@pytest.mark.parametrize("dt", DTYPES)
def test_buckets_are_announced_where_they_were(dry_run, dt):
    notes, total = _on_ready_notes(dt)
    assert notes == ON_READY_PARENT[dt]
    assert notes[-1][0] == total            # the last bucket follows the last launch of the list
