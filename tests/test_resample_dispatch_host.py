"""The dispatch of csrc/resample.hip's x2 entry points, asked through srganfd_resample_describe alone (no GPU, made-up addresses, nothing
launched or dereferenced): the table holds exactly the labels tests/test_resample_gpu.py asserts, and each threshold between two kernels
flips the label at the value the source states."""
import pytest

from tests import test_resample_gpu as G

P = 4096                                                     # a non-null, 16-byte aligned address
DT = ["f32", "bf16", "f16"]


@pytest.fixture()
def describe():
    from sr_gan_fd_amd import _abi as A, ops
    code = {"f32": A.F32, "bf16": A.BF16, "f16": A.F16}
    V = lambda cs=64, c0=0, p=P: A.View(p, cs, c0, 0, 0)

    def d(dt, n, h, w, c, op=None, a=None, b=None, **kw):
        a, b = a or V(), b or V()
        if op is None:
            kw = dict(act=kw.get("act") or V(), b2=kw.get("b2") or V())
        label, _, got_dt = ops.resample_describe(code[dt], n, h, w, c, a, b, op, **kw).rpartition("/")
        assert got_dt == dt
        return label
    d.V, d.A = V, A
    A.set_dry_run(True)
    try:
        yield d
    finally:
        A.set_dry_run(False)


def vn(dt):
    return 4 if dt == "f32" else 8


@pytest.mark.parametrize("dt", DT)
def test_the_table_holds_the_thirteen_labels_and_no_other(describe, dt):
    d, V = describe, describe.V
    seen = set()
    for op in range(5):
        seen.add(d(dt, 2, 4, 4, 32, op))                                 # 16-byte views
        seen.add(d(dt, 2, 4, 4, 32, op, a=V(c0=2)))                      # a view that is none
        seen.add(d(dt, 1, 65536, 1, 32, op))                             # too tall for the row grid
    seen.add(d(dt, 2, 4, 4, 32))                                         # the fused entry: plain, non-temporal, too tall
    seen.add(d(dt, 6, 512, 512, (192 << 20) // (6 * 512 * 512 * (4 if dt == "f32" else 2))))
    seen.add(d(dt, 1, 65536, 1, 32))
    assert len(G.LABELS) == 13 and sorted(seen) == G.LABELS, (sorted(seen - set(G.LABELS)), sorted(set(G.LABELS) - seen))


@pytest.mark.parametrize("dt", DT)
def test_views_that_are_no_16_byte_vectors_take_the_scalar_forms(describe, dt):
    d, V, k = describe, describe.V, vn(dt)
    for op in range(5):
        assert d(dt, 2, 4, 4, 4 * k, op) == G.VECTOR[op]
        assert d(dt, 2, 4, 4, 4 * k - 1, op) == G.SCALAR[op] == d(dt, 2, 4, 4, 3, op)              # c
        for v in (V(c0=k), V(cs=64 + k)):                                                        # one vector further: still vectors
            assert d(dt, 2, 4, 4, 4 * k, op, a=v) == d(dt, 2, 4, 4, 4 * k, op, b=v) == G.VECTOR[op]
        for v in (V(c0=k // 2), V(c0=1), V(cs=64 + k // 2), V(p=P + 8)):                         # c0, cstride, the address
            assert d(dt, 2, 4, 4, 4 * k, op, a=v) == d(dt, 2, 4, 4, 4 * k, op, b=v) == G.SCALAR[op]
    # the fused entry has no scalar form: it refuses
    for bad in (dict(a=V(c0=k // 2)), dict(b=V(c0=1)), dict(act=V(cs=64 + k // 2)), dict(b2=V(p=P + 8))):
        with pytest.raises(describe.A.SrganfdError, match="16-byte"):
            d(dt, 2, 4, 4, 4 * k, **bad)
    with pytest.raises(describe.A.SrganfdError, match="16-byte"):
        d(dt, 2, 4, 4, 4 * k - 1)


@pytest.mark.parametrize("dt", DT)
def test_the_row_grid_ends_where_a_grid_or_the_32_bit_column_decode_ends(describe, dt):
    d, k = describe, vn(dt)
    for op, fused in ((1, False), (2, False), (None, True)):
        rows, generic = (G.VECTOR[2], G.GENERIC[2]) if fused else (G.VECTOR[op], G.GENERIC[op])
        assert d(dt, 1, 65535, 1, 32, op) == rows and d(dt, 1, 65536, 1, 32, op) == generic       # rows: blockIdx.y
        assert d(dt, 65535, 1, 1, 32, op) == rows and d(dt, 65536, 1, 1, 32, op) == generic       # images: blockIdx.z
        w = 2 ** 31 // 2                                                                         # w * (c / vn) = 2^31 with two vectors
        wide = G.ROWS_BWD_NT if fused else rows                                                  # a row of 32 GiB: far past 192 MiB
        assert d(dt, 1, 1, w - 1, 2 * k, op) == wide and d(dt, 1, 1, w, 2 * k, op) == generic
    for op in (0, 3, 4):                                                                         # one form whatever the height
        assert d(dt, 1, 65536, 1, 32, op) == d(dt, 1, 4, 1, 32, op) == G.VECTOR[op]


@pytest.mark.parametrize("dt", DT)
def test_results_of_192_mib_leave_the_fused_entry_through_nontemporal_stores(describe, dt):
    """a result is whole 16-byte vectors, so the largest one under 192 MiB ends 16 bytes under it"""
    d = describe
    vectors = (192 << 20) // 16
    for n, h, w in ((1, 1, vectors), (6, 512, 512 * 64 * 2 // 16), (3, 2 ** 11, 2 ** 11)):
        assert n * h * w == vectors
        assert d(dt, n, h, w, vn(dt)) == G.ROWS_BWD_NT
        assert d(dt, n, h, w, vn(dt), 2) == G.VECTOR[2]                                            # srganfd_resample's op 2 never does
    assert d(dt, 1, 1, vectors - 1, vn(dt)) == G.VECTOR[2]
    assert d(dt, 1, 1, vectors // 2, 2 * vn(dt)) == G.ROWS_BWD_NT and d(dt, 1, 1, vectors // 2 - 1, 2 * vn(dt)) == G.VECTOR[2]


def test_describe_refuses_what_the_entry_points_refuse(describe):
    d, V, A = describe, describe.V, describe.A
    from sr_gan_fd_amd import ops
    for op in (5, -1):
        with pytest.raises(A.SrganfdError, match="bad op"):
            d("f16", 2, 4, 4, 32, op)
    with pytest.raises(A.SrganfdError, match="planar"):
        d("f16", 2, 4, 4, 32, 1, a=A.View(P, 64, 0, 1, 0))
    with pytest.raises(A.SrganfdError, match="cstride"):
        d("f16", 2, 4, 4, 32, 1, b=V(c0=40))
    with pytest.raises(A.SrganfdError, match="null view"):
        ops.resample_describe(A.F16, 2, 4, 4, 32, V(), V())                # the fused entry without act and dx_masked
    with pytest.raises(A.SrganfdError, match="bad dtype"):
        ops.resample_describe(99, 2, 4, 4, 32, V(), V(), 1)
    buf_less = A.lib().srganfd_resample_describe(0, 1, V(), V(), A.NULL_VIEW, A.NULL_VIEW, A.F16, 2, 4, 4, 32, None, 0)
    assert buf_less == -1 and b"no buffer" in A.lib().srganfd_last_error()
    assert A.lib().srganfd_resample_describe(2, 1, V(), V(), A.NULL_VIEW, A.NULL_VIEW, A.F16, 2, 4, 4, 32, b" " * 8, 8) == -1
