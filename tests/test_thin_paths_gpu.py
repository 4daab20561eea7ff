"""Every instantiation and argument combination of csrc/conv_thin.hip through the C ABI against tests/thin_oracle.py in float64, element by
element (thin_oracle's docstring states the bounds).  The kernels get the UNROUNDED fp32 weight, the oracle ``W.to(dt)``.  Every case
also asserts the kernel label (ops.thin_describe) and that nothing outside the output view was written (sentinels around NHWC slices,
planar groups, fp32 outputs and gradients); thin_wgrad is run twice and must repeat bit for bit.

The case tables are plain data; tests/test_thin_oracle_host.py holds the labels they reach against the 12 labelled instantiations.
SRGANFD_THIN_PATHS_REPORT=<file> writes the worst err / bound per kernel label there (profiles/conv_thin_paths_fp64.txt is such a run).

Shapes (n, h, w): one and three tile columns of both strip widths (thin_in 64 = 4 x 16, thin_out 56 = 4 x 14 columns), a second tile row of a
single row (33 rows), odd row counts against the read-ahead depths 2 and 4, and one pixel."""
import os

import pytest
import torch

from tests import conv_oracle as O
from tests import thin_oracle as T

HALF = (torch.bfloat16, torch.float16)
NAME = {torch.bfloat16: "bf16", torch.float16: "f16"}
F32 = torch.float32
SHAPES = [(2, 16, 16), (1, 37, 52), (2, 33, 70), (1, 64, 129), (3, 5, 7), (1, 1, 1)]
CS = (1, 2, 3, 4)
# thin_in stores non-temporally from this many bytes of n * h * w * big.cstride 16-bit elements (kThinNtBytes in csrc/conv_thin.hip)
NT_BYTES = 192 << 20
NT_SHAPE = (2, 33, 70)
SLAB_BYTES = 4 * 3088               # one workgroup's slab of thin_wgrad's workspace: the workspace query / this = its grid

# where the 64-channel tensor lives: (channels of the buffer, first channel of the view, planar)
DENSE, SLICE96, SLICE128, PLANAR192 = (64, 0, 0), (96, 32, 0), (128, 32, 0), (192, 64, 1)

# ---- thin_in: name -> (w_big_is_cout, flip, bias, act, mask layout or None, output layout) ----
IN_MODES = {
    "fwd_lrelu": (1, 0, True, O.ACT_LRELU, None, SLICE96),
    "fwd_relu": (1, 0, True, O.ACT_RELU, None, PLANAR192),
    "fwd_plain": (1, 0, False, O.ACT_NONE, None, DENSE),
    "dgrad_mask": (0, 1, False, O.ACT_NONE, DENSE, SLICE96),
    "dgrad_mask_planar": (0, 1, False, O.ACT_NONE, PLANAR192, PLANAR192),
    "dgrad_mask_slice": (0, 1, False, O.ACT_NONE, SLICE96, DENSE),
    "dgrad_plain": (0, 1, False, O.ACT_NONE, None, DENSE),
}
IN_CASES = [(m, cs) for m in IN_MODES for cs in CS]
# the non-temporal twins: (masked, channels of the output buffer) -- 2 x 33 x 70 pixels in a buffer wide enough to pass NT_BYTES, and one
# just under it that must take the plain kernel
NT_CASES = [(False, 21792, True), (True, 21792, True), (True, 21784, False)]

# ---- thin_out: (name, w_big_is_cout, flip, bias, pitch, input layout), every one for cs 1..4 where the pitch allows ----
OUT_MODES = {
    "fwd_bias": (0, 0, True, 4, DENSE),
    "fwd_nobias_slice": (0, 0, False, 4, SLICE128),
    "dgrad": (1, 1, False, 4, DENSE),
    "fwd_bias_pitch1_slice": (0, 0, True, 1, SLICE128),
}
OUT_CASES = [(m, cs) for m in OUT_MODES for cs in CS if OUT_MODES[m][3] == 4 or cs == 1]

# ---- thin_wgrad: operand layout x whether db is asked for, for both orientations and cs 1..4 ----
WG_MODES = {"nhwc": (DENSE, True), "slice_nodb": (SLICE96, False), "planar": (PLANAR192, True), "planar_nodb": (PLANAR192, False)}
WG_CASES = [(m, cs, bic) for m in WG_MODES for cs in CS for bic in (1, 0)]


def in_label(dt, masked, nt=False):
    return "thin_in_kernel<%s%s%s>" % (NAME[dt], ",mask" if masked else "", ",NT" if nt else "")


def out_label(dt):
    return "thin_out_kernel<%s>" % NAME[dt]


def wg_label(dt):
    return "thin_wgrad_kernel<%s>" % NAME[dt]


def thin_args(dt, shape, cs, layout, *, w_big_is_cout, flip=0, bias=None, act=O.ACT_NONE, mask_layout=None, pitch=4, ptrs=None):
    """the launch struct; ``ptrs`` = dict(weight, big, bias, mask, thin, thin_out) of device addresses, or None for 16-byte-aligned dummies
    (enough for ops.thin_describe in dry-run mode, which launches nothing)"""
    from sr_gan_fd_amd import _abi as A, ops
    n, h, w = shape
    p = ptrs or dict(weight=0x10000, big=0x20000, bias=0x30000, mask=0x40000, thin=0x50000, thin_out=0x60000)
    cbuf, c0, planar = layout
    mask = A.View(p["mask"], mask_layout[0], mask_layout[1], mask_layout[2], 0) if mask_layout else A.NULL_VIEW
    return ops.thin_args(ops.DT[dt], n, h, w, cs, p["weight"], A.View(p["big"], cbuf, c0, planar, 0), w_big_is_cout=bool(w_big_is_cout), flip=bool(flip),
                         bias=p["bias"] if bias else None, act=act, slope=0.2, mask=mask, mask_slope=0.2, thin=p["thin"], thin_out=p["thin_out"],
                         thin_out_pitch=pitch)


def wgrad_units_shape(ws_bytes):
    """(n, h, w) at which some waves of thin_wgrad's persistent grid run three units and the rest two: width 33 = two column blocks per
    row, the second with one valid column, and n * h * 2 units > 2 * waves"""
    waves = 8 * (ws_bytes // SLAB_BYTES)
    return waves // 520 + 1, 520, 33


def dummy_launches():
    """(launch struct, op, expected label) of every case of the tables, with dummy pointers"""
    out = []
    for dt in HALF:
        for shape in SHAPES:
            for m, cs in IN_CASES:
                bic, flip, bias, act, ml, lay = IN_MODES[m]
                out.append((thin_args(dt, shape, cs, lay, w_big_is_cout=bic, flip=flip, bias=bias, act=act, mask_layout=ml), 0, in_label(dt, ml is not None)))
            for m, cs in OUT_CASES:
                bic, flip, bias, pitch, lay = OUT_MODES[m]
                out.append((thin_args(dt, shape, cs, lay, w_big_is_cout=bic, flip=flip, bias=bias, pitch=pitch), 1, out_label(dt)))
            for m, cs, bic in WG_CASES:
                out.append((thin_args(dt, shape, cs, WG_MODES[m][0], w_big_is_cout=bic), 2, wg_label(dt)))
        for masked, cbuf, nt in NT_CASES:
            out.append((thin_args(dt, NT_SHAPE, 3, (cbuf, 64, 0), w_big_is_cout=not masked, flip=masked, mask_layout=DENSE if masked else None), 0,
                        in_label(dt, masked, nt)))
    return out


# ---- the GPU side ----
RATIOS = {}            # kernel label -> worst err / bound seen


def _record(lab, ratio):
    RATIOS[lab] = max(RATIOS.get(lab, 0.0), ratio)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    lines = [f"{r:8.4f}  {lab}" for lab, r in sorted(RATIOS.items())]
    print("\nworst err / bound per kernel label\n" + "\n".join(lines))
    path = os.environ.get("SRGANFD_THIN_PATHS_REPORT")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


_DATA = {}             # (dtype, shape, cs) -> the operands on the host, drawn once and shared by every case of that shape
_REFS = {}             # what a case computes from them in float64, shared by the cases that differ in layout only


def _data(dt, shape, cs):
    key = (dt, shape, cs)
    if key not in _DATA:
        if len(_DATA) > 64:
            _DATA.clear()
            _REFS.clear()
        n, h, w = shape
        g = torch.Generator().manual_seed(4321 + 13 * cs + h * w)
        rnd = lambda *s: torch.randn(*s, generator=g)
        thin = torch.zeros(n, h, w, 4, dtype=dt)
        thin[..., :cs] = rnd(n, h, w, cs).to(dt)
        _DATA[key] = dict(thin=thin, big=rnd(n, h, w, 64).to(dt), mask=rnd(n, h, w, 64).to(dt), w_in=rnd(64, cs, 3, 3) * 0.3, w_out=rnd(cs, 64, 3, 3) * 0.1,
                          b64=rnd(64), bcs=rnd(cs))
    return _DATA[key]


def _ref(key, fn):
    if key not in _REFS:
        _REFS[key] = fn()
    return _REFS[key]


def _big_buf(shape, layout, dt, data=None):
    """the 64-channel tensor inside its buffer: ``data`` at the view's channels and garbage elsewhere (an input), or all sentinel (an output)"""
    n, h, w = shape
    cbuf, c0, planar = layout
    b = O.Buf(n, h, w, cbuf, dt, planar, fill="sentinel" if data is None else "garbage", gen=torch.Generator().manual_seed(7))
    if data is not None:
        b.put(c0, data)
    return b.upload()


class Guarded:
    """an fp32 device tensor of ``shape`` inside a flat buffer with 64 sentinel floats before and after it"""

    def __init__(self, shape):
        numel = 1
        for s in shape:
            numel *= s
        self.flat = torch.full((numel + 128,), O.SENTINEL, dtype=F32, device="cuda")
        self.val = self.flat[64:64 + numel].view(shape)

    def assert_guards(self, what):
        assert bool((self.flat[:64] == O.SENTINEL).all()) and bool((self.flat[-64:] == O.SENTINEL).all()), f"{what}: written outside the tensor"


def _check_label(a, op, lab):
    from sr_gan_fd_amd import ops
    got = ops.thin_describe(a, op)
    assert got == lab, (got, lab)


def _ptrs(**t):
    return {k: (v.data_ptr() if v is not None else None) for k, v in t.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("dt", HALF, ids=NAME.get)
@pytest.mark.parametrize("mode,cs", IN_CASES, ids=lambda v: str(v))
def test_thin_in(dt, mode, cs):
    from sr_gan_fd_amd import _abi as A, ops
    bic, flip, bias, act, ml, lay = IN_MODES[mode]
    lab = in_label(dt, ml is not None)
    for shape in SHAPES:
        D = _data(dt, shape, cs)
        W = D["w_in"] if bic else D["w_out"]
        ref, mag = _ref(("in", dt, shape, cs, bic, flip, bias, act, ml is not None),
                        lambda: T.thin_in(D["thin"], W.to(dt), cs, w_big_is_cout=bic, flip=flip, bias=D["b64"] if bias else None, act=act, slope=O_f32(0.2),
                                          mask=D["mask"] if ml else None, mask_slope=O_f32(0.2)))
        out = _big_buf(shape, lay, dt)
        msk = _big_buf(shape, ml, dt, D["mask"]) if ml else None
        dev = dict(weight=W.cuda(), bias=D["b64"].cuda(), thin=D["thin"].cuda())
        a = thin_args(dt, shape, cs, lay, w_big_is_cout=bic, flip=flip, bias=bias, act=act, mask_layout=ml,
                      ptrs=_ptrs(big=out.dev, mask=msk.dev if msk else None, thin_out=None, **dev))
        _check_label(a, 0, lab)
        ops.thin_in(a)
        torch.cuda.synchronize()
        got = out.download()
        what = f"thin_in {mode} cs {cs} {NAME[dt]} {shape}"
        out.assert_outside_untouched(got, lay[1], 64, what)
        ratio, at = T.ratio_in(got[..., lay[1]:lay[1] + 64], ref, mag, cs, dt, ml is not None)
        print(f"{what}: worst err / bound {ratio:.4f}  [{lab}]")
        assert ratio <= 1.0, f"{what}: element {at} is {ratio:.3f} times its bound"
        _record(lab, ratio)


def O_f32(v):
    """the float32 the struct carries"""
    return float(torch.tensor(v, dtype=F32))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", HALF, ids=NAME.get)
@pytest.mark.parametrize("masked,cbuf,nt", NT_CASES, ids=lambda v: str(v))
def test_thin_in_non_temporal(dt, masked, cbuf, nt):
    """the NT = true instantiations (what every full-size training step runs) at a small image: the output view is 64 channels of a buffer
    wide enough that n * h * w * cstride * 2 passes the threshold; the sentinel check over the whole buffer runs on the device"""
    from sr_gan_fd_amd import ops
    shape, cs, c0 = NT_SHAPE, 3, 64
    n, h, w = shape
    assert (n * h * w * cbuf * 2 >= NT_BYTES) == nt and n * h * w * (cbuf + 8) * 2 >= NT_BYTES       # the pair straddles the threshold
    D = _data(dt, shape, cs)
    W = D["w_out"] if masked else D["w_in"]
    ref, mag = _ref(("in", dt, shape, cs, int(not masked), int(masked), False, O.ACT_NONE, masked),
                    lambda: T.thin_in(D["thin"], W.to(dt), cs, w_big_is_cout=not masked, flip=masked, mask=D["mask"] if masked else None, mask_slope=O_f32(0.2)))
    buf = torch.full((n, h, w, cbuf), O.SENTINEL, dtype=dt, device="cuda")
    msk = D["mask"].cuda() if masked else None
    dev = dict(weight=W.cuda(), thin=D["thin"].cuda())
    a = thin_args(dt, shape, cs, (cbuf, c0, 0), w_big_is_cout=not masked, flip=masked, mask_layout=DENSE if masked else None,
                  ptrs=_ptrs(big=buf, mask=msk, bias=None, thin_out=None, **dev))
    lab = in_label(dt, masked, nt)
    _check_label(a, 0, lab)
    ops.thin_in(a)
    torch.cuda.synchronize()
    what = f"thin_in non-temporal {nt} masked {masked} {NAME[dt]}"
    assert bool((buf[..., :c0] == O.SENTINEL).all()) and bool((buf[..., c0 + 64:] == O.SENTINEL).all()), f"{what}: written outside the view"
    ratio, at = T.ratio_in(buf[..., c0:c0 + 64].cpu(), ref, mag, cs, dt, masked)
    print(f"{what}: worst err / bound {ratio:.4f}  [{lab}]")
    assert ratio <= 1.0, f"{what}: element {at} is {ratio:.3f} times its bound"
    _record(lab, ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", HALF, ids=NAME.get)
@pytest.mark.parametrize("mode,cs", OUT_CASES, ids=lambda v: str(v))
def test_thin_out(dt, mode, cs):
    from sr_gan_fd_amd import ops
    bic, flip, bias, pitch, lay = OUT_MODES[mode]
    lab = out_label(dt)
    for shape in SHAPES:
        n, h, w = shape
        D = _data(dt, shape, cs)
        W = D["w_in"] if bic else D["w_out"]
        ref, mag = _ref(("out", dt, shape, cs, bic, flip, bias),
                        lambda: T.thin_out(D["big"], W.to(dt), cs, w_big_is_cout=bic, flip=flip, bias=D["bcs"] if bias else None))
        src = _big_buf(shape, lay, dt, D["big"])
        out = Guarded((n, h, w, pitch))
        dev = dict(weight=W.cuda(), bias=D["bcs"].cuda())
        a = thin_args(dt, shape, cs, lay, w_big_is_cout=bic, flip=flip, bias=bias, pitch=pitch, ptrs=_ptrs(big=src.dev, mask=None, thin=None, thin_out=out.val, **dev))
        _check_label(a, 1, lab)
        ops.thin_out(a)
        torch.cuda.synchronize()
        what = f"thin_out {mode} cs {cs} {NAME[dt]} {shape}"
        out.assert_guards(what)
        got = out.val.cpu()
        if pitch == 4 and cs < 4:
            assert bool((got[..., cs:] == 0).all()), f"{what}: channels >= cs are not zeros"
        ratio, at = O.worst_ratio(got[..., :cs], ref, mag, 9 * 64, F32)
        print(f"{what}: worst err / bound {ratio:.4f}  [{lab}]")
        assert ratio <= 1.0, f"{what}: element {at} is {ratio:.3f} times its bound"
        _record(lab, ratio)


def _run_wgrad(dt, shape, cs, bic, lay, with_db, ws, what):
    from sr_gan_fd_amd import ops
    n, h, w = shape
    D = _data(dt, shape, cs)
    dw_ref, db_ref, A_dw, A_db = _ref(("wg", dt, shape, cs, bic), lambda: T.thin_wgrad(D["big"], D["thin"], cs, w_big_is_cout=bic))
    src = _big_buf(shape, lay, dt, D["big"])
    wshape = (64, cs, 3, 3) if bic else (cs, 64, 3, 3)
    dev = dict(weight=torch.zeros(wshape, device="cuda"), thin=D["thin"].cuda())
    a = thin_args(dt, shape, cs, lay, w_big_is_cout=bic, ptrs=_ptrs(big=src.dev, mask=None, bias=None, thin_out=None, **dev))
    lab = wg_label(dt)
    _check_label(a, 2, lab)
    runs = []
    for _ in range(2):
        dw, db = Guarded(wshape), Guarded((64 if bic else cs,))
        ops.thin_wgrad(a, dw.val, db.val if with_db else None, ws)
        torch.cuda.synchronize()
        dw.assert_guards(what + " dw")
        db.assert_guards(what + " db")
        runs.append((dw.val.cpu(), db.val.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), f"{what}: not bitwise run-to-run"
    K = n * h * w
    ratio, at = O.worst_ratio(runs[0][0], dw_ref, A_dw, K, F32)
    if with_db:
        rb, atb = O.worst_ratio(runs[0][1], db_ref, A_db, K, F32)
        ratio, at = max((ratio, at), (rb, atb))
    else:
        assert bool((runs[0][1] == O.SENTINEL).all()), f"{what}: db == NULL, yet the would-be bias gradient was written"
    print(f"{what}: worst err / bound {ratio:.4f}  [{lab}]")
    assert ratio <= 1.0, f"{what}: element {at} is {ratio:.3f} times its bound"
    _record(lab, ratio)


@pytest.fixture(scope="module")
def wgrad_ws():
    from sr_gan_fd_amd import ops
    return torch.empty(ops.thin_wgrad_workspace_bytes(), dtype=torch.uint8, device="cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", HALF, ids=NAME.get)
@pytest.mark.parametrize("mode,cs,bic", WG_CASES, ids=lambda v: str(v))
def test_thin_wgrad(dt, mode, cs, bic, wgrad_ws):
    lay, with_db = WG_MODES[mode]
    for shape in SHAPES:
        _run_wgrad(dt, shape, cs, bic, lay, with_db, wgrad_ws, f"thin_wgrad {mode} cs {cs} big_is_cout {bic} {NAME[dt]} {shape}")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", HALF, ids=NAME.get)
@pytest.mark.parametrize("bic", (1, 0))
def test_thin_wgrad_several_units_per_wave(dt, bic, wgrad_ws):
    """the persistent loop: load_unit(u + nw) behind the commit of unit u, and the overwrite of the wave-private LDS image that the
    previous unit's transposing reads used -- some waves run three units, the rest two"""
    shape = wgrad_units_shape(wgrad_ws.numel())
    n, h, w = shape
    waves = 8 * (wgrad_ws.numel() // SLAB_BYTES)
    assert n * h * 2 > 2 * waves and n * h * 2 < 3 * waves
    _run_wgrad(dt, shape, 3, bic, DENSE, True, wgrad_ws, f"thin_wgrad {shape} = {n * h * 2} units on {waves} waves, big_is_cout {bic} {NAME[dt]}")
