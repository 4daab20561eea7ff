"""csrc/conv_igemm.hip against the float64 formula of tests/conv_oracle.py on every dispatch path: (a) the persistent-tile loop of the
kind-0 16-bit 3x3 kernels (workgroups that run two and three tiles, with the channel block, the weight block and the bias changing
between them), (b) every instantiation reachable below the non-temporal threshold, with every epilogue operand, in NHWC and planar
views.

Criterion (conv_oracle.bound), for EVERY stored element of y and y2:
    |got - ref| <= u |ref| + 4 (K + 8) 2^-24 A + 2^-24,    K = ksize^2 cin, u = 2^-8 (bf16) / 2^-11 (f16) / 2^-24 (fp32 output, f32 mode)
A = the formula on absolute values.  Every case also asserts the kernel label it expects and that nothing outside the output view
(NHWC or planar) was written.  The case tables are plain data: tests/test_conv_oracle_host.py builds the same launches with dummy
pointers and holds the set of labels they reach against the list of instantiations in dispatch_conv.

SRGANFD_CONV_PATHS_REPORT=<file> writes the worst err / bound per kernel label there (profiles/conv_paths_fp64.txt is such a run).
"""
import os

import pytest
import torch

from tests import conv_oracle as O

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
ALL, HALF = (F32, BF16, F16), (BF16, F16)
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
CINS = (32, 96)
WOUT = 37

# tile (MR, WR, WN) of (ksize, stride, wide): a workgroup's tile is MR * WR rows x 32 pixels x 32 * WN channels
TILE16 = {(3, 1, 1): (2, 4, 2), (3, 1, 0): (2, 8, 1), (3, 2, 1): (1, 4, 2), (3, 2, 0): (1, 4, 1), (2, 1, 1): (2, 4, 2), (2, 1, 0): (2, 8, 1),
          (4, 2, 1): (1, 4, 2), (4, 2, 0): (1, 4, 1), (2, 2, 1): (1, 4, 2), (2, 2, 0): (1, 4, 1), (1, 1, 1): (2, 4, 1), (1, 1, 0): (2, 4, 1)}
TILE32 = dict(TILE16)
TILE32[(4, 2, 1)] = (1, 4, 1)           # f32: the stride-2 patch of a 4x4 kernel fits a 32-channel tile only


def f32r(v):
    """a scalar argument as the fp32 the launch struct holds"""
    return float(torch.tensor(float(v), dtype=torch.float32))


def label(dtype, k, s, wide, ek=None, cls=False):
    """the kernel label expected of (element type, kernel shape, tile width, fixed epilogue kind, class launch)"""
    mr, wr, wn = (TILE32 if dtype == F32 else TILE16)[(k, s, int(wide))]
    half = dtype != F32
    ts = ",TS=2" if half and (k, s, int(wide)) == (4, 2, 1) else ""
    eks = f",E{ek}" if half and ek is not None else ""
    return f"conv_igemm_kernel<{NAME[dtype]},KS={k},S={s},MR={mr},WR={wr},WN={wn}{',M16' if half else ''}{ts}{eks}>{'[4 classes]' if cls else ''}"


DEFAULTS = dict(k=3, s=1, p=1, up=0, cout=64, cout_store=None, y_f32=False, bias=False, act=O.ACT_NONE, slope=0.2, alpha=1.0, alpha_dev=None,
                post_scale=1.0, r1=None, r2=None, mask=None, y2=False, y2_other=False, y_c0=32, transposed=False, form=None, ek=None,
                planar=(0, 1), dtypes=ALL)

# ---- (b) every small-shape instantiation, every operand.  r1 / r2: the scale; mask: the mask_slope; ek: the fixed epilogue kind the
# 16-bit 3x3 stride-1 launch must take (None: the run-time epilogue) ----
SMALL = [
    # 3x3 stride 1, 64-channel tiles: the four fixed kinds, then the run-time vector epilogue with y2
    dict(name="k3_wide_E0", bias=True, act=O.ACT_LRELU, slope=0.1, alpha=1.5, post_scale=0.5, ek=0),
    dict(name="k3_wide_E0_relu", bias=True, act=O.ACT_RELU, ek=0),
    dict(name="k3_wide_E1", bias=True, r1=0.2, alpha=0.75, post_scale=0.4, ek=1),
    dict(name="k3_wide_E3", bias=True, r1=0.2, r2=1.0, alpha=1.25, post_scale=0.04, ek=3),
    dict(name="k3_wide_E4_mask_no_act", mask=0.2, ek=4),
    dict(name="k3_wide_y2_r1_r2_mask", bias=True, act=O.ACT_LRELU, alpha=1.5, alpha_dev=0.6, post_scale=0.8, r1=0.5, r2=-1.0, mask=0.25, y2=True),
    dict(name="k3_wide_y2_other_layout", bias=True, act=O.ACT_RELU, r1=1.0, y2=True, y2_other=True),
    dict(name="k3_wide_128", cout=128, bias=True, act=O.ACT_LRELU, ek=0),                       # two channel blocks
    # 3x3 stride 1, 32-channel tiles: kind 0 leaves through the transposed 16-bit row tiles
    dict(name="k3_narrow_E0", cout=32, bias=True, act=O.ACT_LRELU, alpha=1.5, post_scale=0.5, ek=0),
    dict(name="k3_narrow_E0_relu", cout=32, act=O.ACT_RELU, ek=0),
    dict(name="k3_narrow_E4", cout=32, mask=0.1, ek=4),
    dict(name="k3_narrow_y2_r1", cout=32, bias=True, act=O.ACT_LRELU, slope=0.1, alpha=2.0, alpha_dev=0.3, r1=0.2, y2=True),
    # the scalar epilogue: partial channels + fp32 output, an unaligned view, fp32 output of a wide tile
    dict(name="k3_scalar_store3_f32out", cout=32, cout_store=3, y_f32=True, bias=True, act=O.ACT_LRELU, alpha=1.5, post_scale=0.5,
         r1=0.2, r2=1.0, mask=0.2, y2=True, planar=(0,)),
    dict(name="k3_scalar_unaligned", y_c0="unaligned", bias=True, act=O.ACT_LRELU, slope=0.1, r1=0.2, r2=0.5, mask=0.2, y2=True, planar=(0,)),
    dict(name="k3_scalar_f32out_relu", y_f32=True, bias=True, act=O.ACT_RELU, alpha_dev=1.75, planar=(0,)),
    # nearest x2 folded into the gather; the data-gradient orientation
    dict(name="k3_up", up=1, bias=True, act=O.ACT_LRELU, ek=0),
    dict(name="k3_dgrad_mask", cout=32, transposed=True, mask=0.2, ek=4),
    dict(name="k3_dgrad_wide_r1", transposed=True, r1=1.0, ek=1),
    # the other kernel shapes, forward
    dict(name="k3s2_wide", s=2, bias=True, act=O.ACT_LRELU, alpha_dev=0.7),
    dict(name="k3s2_narrow", s=2, cout=32, bias=True, r1=0.2, y2=True),
    dict(name="k4s2_wide", k=4, s=2, bias=True, act=O.ACT_LRELU, alpha=1.5, alpha_dev=0.8),
    dict(name="k4s2_narrow", k=4, s=2, cout=32, mask=0.2),
    dict(name="k2s2_wide", k=2, s=2, p=0, bias=True, act=O.ACT_RELU),
    dict(name="k2s2_narrow", k=2, s=2, p=0, cout=32, bias=True, r1=1.0),
    dict(name="k2s1_wide", k=2, bias=True, act=O.ACT_LRELU),
    dict(name="k2s1_narrow", k=2, cout=32, bias=True, mask=0.2),
    dict(name="k1", k=1, p=0, cout=32, bias=True, act=O.ACT_LRELU, slope=0.1),
    dict(name="k1_two_blocks_y2", k=1, p=0, bias=True, r1=0.5, y2=True),
    # the data gradient of the stride-2 convs as output-parity classes: four single-class launches and, 16-bit, out_classes = 4
    dict(name="cls_k4s2_wide_r1", form="k4s2", r1=1.0),
    dict(name="cls_k4s2_narrow_mask", form="k4s2", cout=32, mask=0.2),
    dict(name="cls_k3s2_wide_mask", form="k3s2", mask=0.2),
    dict(name="cls_k3s2_narrow", form="k3s2", cout=32),
    dict(name="cls_k2s2_r1", form="k2s2", r1=1.0),
]
SMALL = [dict(DEFAULTS, **c) for c in SMALL]


def small_id(p):
    case, dtype, cin, planar = p
    return f"{case['name']}-{NAME[dtype]}-cin{cin}-{'planar' if planar else 'nhwc'}"


SMALL_PARAMS = [(c, dt, cin, pl) for c in SMALL for dt in c["dtypes"] for cin in CINS for pl in c["planar"]]


# ---- (a) persistent tiles: kind 0, 16-bit, both tile shapes; the image is 17 x 40 (a full, a ragged-row and a ragged-column tile) ----
PH, PW = 17, 40
_PERS = dict(DEFAULTS, bias=True, act=O.ACT_LRELU, alpha=1.5, post_scale=0.5, ek=0, dtypes=HALF, planar=(0,))
PERSISTENT = [
    # Three channel blocks: a workgroup's tiles v, v + grid, ... are blocks xcd_remap(v) + grid / 8 apart, and their channel block is
    # that index modulo cout / NB -- with 1, 2 or 4 channel blocks and a grid of 512 every tile of a workgroup has the SAME channel
    # block.  With 3 the weight descriptor and the bias registers change from tile to tile (the test asserts that they do).
    dict(_PERS, name="wide_64_192", cin=64, cout=192, changes_block=True),
    dict(_PERS, name="narrow_64_96", cin=64, cout=96, shared=True, planar=(0, 1), changes_block=True),
    dict(_PERS, name="wide_64_128", cin=64, cout=128),                     # two channel blocks
    dict(_PERS, name="wide_32_64", cin=32),                                # one chunk: the next tile is requested in the tile's only chunk
    dict(_PERS, name="wide_96_64", cin=96),                                # odd chunk count
    dict(_PERS, name="wide_64_128_relu", cin=64, cout=128, bias=False, act=O.ACT_RELU, alpha=1.0, post_scale=1.0),
    # x and y are slices of ONE 192-channel buffer (a dense block's): channels [0, cin) in, [cin, cin + 32) out
    dict(_PERS, name="narrow_64_32", cin=64, cout=32, shared=True, planar=(0, 1)),
    dict(_PERS, name="narrow_32_32", cin=32, cout=32, shared=True, planar=(0, 1)),
    dict(_PERS, name="narrow_160_32", cin=160, cout=32, shared=True, planar=(0, 1)),
    dict(_PERS, name="narrow_64_32_relu", cin=64, cout=32, shared=True, planar=(0, 1), bias=False, act=O.ACT_RELU, alpha=1.0, post_scale=1.0),
    # The kinds with epilogue operands, same sizes: one tile per workgroup in the product library (many more blocks than the chip
    # holds, the uneven arm of xcd_remap), persistent in a -DSRGANFD_CROSS_MASK=0 build selected with SRGANFD_LIB
    dict(_PERS, name="wide_64_192_E1", cin=64, cout=192, changes_block=True, r1=0.2, ek=1),
    dict(_PERS, name="wide_64_192_E3", cin=64, cout=192, changes_block=True, r1=0.2, r2=1.0, ek=3),
    dict(_PERS, name="wide_64_192_E4", cin=64, cout=192, changes_block=True, bias=False, act=O.ACT_NONE, mask=0.2, ek=4),
    dict(_PERS, name="narrow_64_96_E4", cin=64, cout=96, shared=True, changes_block=True, bias=False, act=O.ACT_NONE, mask=0.2, ek=4),
]
PERSISTENT_PARAMS = [(c, dt, pl) for c in PERSISTENT for dt in c["dtypes"] for pl in c["planar"]]


def persistent_batch(case, cus):
    """(n, nblk, grid) by the host's rule (launch_conv): slots = 2 workgroups per compute unit, grid = slots / 8 * 8 persistent
    workgroups once nblk > slots.  n: the first ODD batch from 2.4 grids of tiles on -- 12 or 4 tiles per image, so nblk is then no
    multiple of 8 -- whose tile count is no multiple of the grid."""
    mr, wr, wn = TILE16[(3, 1, int(case["cout"] % 64 == 0))]
    th, nb = mr * wr, 32 * wn
    per_image = -(-PH // th) * -(-PW // 32) * (case["cout"] // nb)
    slots = 2 * cus
    grid = slots // 8 * 8
    n = -(-int(2.4 * grid) // per_image) | 1
    while n * per_image % grid == 0 or n * per_image % 8 == 0:
        n += 2
    return n, n * per_image, grid


def channel_blocks_of_workgroup(b, nblk, grid, n_nb):
    """the channel block of every tile persistent workgroup b runs: the kernel's decode (conv_common.hpp xcd_remap, then the block
    index modulo the channel blocks)"""
    q, rr = nblk >> 3, nblk & 7
    out = []
    for v in range(b, nblk, grid):
        xcd = v & 7
        bid = (xcd * (q + 1) if xcd < rr else rr * (q + 1) + (xcd - rr) * q) + (v >> 3)
        out.append(bid % n_nb)
    return out


def block_changes(case, nblk, grid):
    n_nb = case["cout"] // (64 if case["cout"] % 64 == 0 else 32)
    return any(len(set(channel_blocks_of_workgroup(b, nblk, grid, n_nb))) > 1 for b in range(0, grid, max(1, grid // 16)))


# ---- one launch plan from a case: shared by the GPU tests (real buffers) and the host label test (dummy pointers) ----
def geometry(case, dtype, cin):
    """(n, h_in, w_in, h_out, w_out, cout) of a small case: the output is (2 TH + 3) x 37 -- interior, ragged-row and ragged-column tiles;
    with up = 1 one more each way (an upsampled size is even).  A class case: (h_in, w_in) is the gradient the classes read and the
    output the full (2 h_in, 2 w_in) image."""
    k, s = (O.CLASS_FORMS[case["form"]][2], 1) if case["form"] else (case["k"], case["s"])
    mr, wr, _ = (TILE32 if dtype == F32 else TILE16)[(k, s, int(case["cout"] % 64 == 0))]
    th = mr * wr
    if case["form"]:
        hd, wd = 2 * th + 3, WOUT
        return 2, hd, wd, 2 * hd, 2 * wd, case["cout"]
    ho, wo = 2 * th + 3 + case["up"], WOUT + case["up"]
    if case["up"]:
        return 2, ho // 2, wo // 2, ho, wo, case["cout"]
    p = case["p"]
    return 2, (ho - 1) * s + k - 2 * p, (wo - 1) * s + k - 2 * p, ho, wo, case["cout"]


def layout(case, dtype, cin, planar, dims):
    """name -> (h, w, cbuf, c0, channels, planar, element type) of every buffer the case's launch has a view of"""
    n, hi, wi, ho, wo, cout = dims
    cs = case["cout_store"] or cout
    y_c0 = (4 if dtype != F32 else 2) if case["y_c0"] == "unaligned" else case["y_c0"]
    if case.get("shared"):
        L = {"x": (hi, wi, 192, 0, cin, planar, dtype), "y": (hi, wi, 192, cin, cs, planar, dtype)}
    else:
        L = {"x": (hi, wi, cin + 64, 32, cin, planar, dtype),
             "y": (ho, wo, 32 + cout + 32, y_c0, cs, planar, F32 if case["y_f32"] else dtype)}
    if case["r1"] is not None:
        L["r1"] = (ho, wo, cout + 32, 32, cs, planar, dtype)
    if case["r2"] is not None:
        L["r2"] = (ho, wo, cout + 64, 0, cs, planar, dtype)
    if case["mask"] is not None:
        L["mask"] = (ho, wo, cout + 32, 32, cs, planar, dtype)
    if case["y2"]:
        L["y2"] = (ho, wo, cout + 64, 0, cs, 1 - planar, dtype) if case["y2_other"] else (ho, wo, cout + 64, 64, cs, planar, dtype)
    return L


def launches(case, dtype, cin, dims, views, wptr, pack_bytes, bias, alpha_dev):
    """[(conv args, expected label, class or None)]: ``views`` name -> srganfd_view; a class case gives the four single-class launches
    (class = 0..3) and, in the 16-bit types, the one out_classes = 4 launch (class = 4)"""
    from sr_gan_fd_amd import ops
    n, hi, wi, ho, wo, cout = dims
    dt = ops.DT[dtype]
    kw = dict(bias=bias, act=case["act"], slope=f32r(case["slope"]), alpha=f32r(case["alpha"]), post_scale=f32r(case["post_scale"]),
              alpha_dev=alpha_dev, mask_slope=0.2)
    for nm in ("r1", "r2"):
        if case[nm] is not None:
            kw.update({nm: views[nm], nm + "_scale": f32r(case[nm])})
    if case["mask"] is not None:
        kw.update(mask=views["mask"], mask_slope=f32r(case["mask"]))
    if case["y2"]:
        kw.update(y2=views["y2"])
    wide = cout % 64 == 0
    if not case["form"]:
        a = ops.conv_args(dt, views["x"], views["y"], wptr, n, hi, wi, cin, cout, cout_store=case["cout_store"], ksize=case["k"], stride=case["s"],
                          pad=case["p"], up=case["up"], y_f32=case["y_f32"], **kw)
        assert (a.h_out, a.w_out) == (ho, wo)
        return [(a, label(dtype, case["k"], case["s"], wide, case["ek"]), None)]
    _, _, kc, _, step, base = O.CLASS_FORMS[case["form"]]
    out = []
    for par in ([0, 1, 2, 3] + ([4] if dtype != F32 else [])):
        a = ops.conv_args(dt, views["x"], views["y"], wptr + (par % 4) * pack_bytes, n, hi, wi, cin, cout, ksize=kc, stride=1, pad=0, **kw)
        a.h_out, a.w_out = hi, wi
        a.out_sy, a.out_sx, a.out_oy, a.out_ox = 2, 2, (par >> 1) & 1, par & 1
        a.out_h_full, a.out_w_full = ho, wo
        a.pad_y, a.pad_x = (base, base) if par == 4 else O.class_pads(case["form"], par)
        a.out_classes, a.class_pad_step = (4, step) if par == 4 else (0, 0)
        out.append((a, label(dtype, kc, 1, wide, cls=par == 4), par))
    return out


def dummy_launches(case, dtype, cin, planar, dims=None):
    """the same launches with 16-byte-aligned non-null dummy pointers: enough for srganfd_conv2d_describe, which launches nothing"""
    from sr_gan_fd_amd import _abi as A
    dims = dims or geometry(case, dtype, cin)
    views = {nm: A.View(0x10000, cbuf, c0, pl, 0) for nm, (_, _, cbuf, c0, _, pl, _) in layout(case, dtype, cin, planar, dims).items()}
    return launches(case, dtype, cin, dims, views, 0x20000, 0x1000, 0x30000 if case["bias"] else None, 0x40000 if case["alpha_dev"] else None)


# ---- the GPU side ----
RATIOS = {}            # kernel label -> worst err / bound seen


def _record(lab, ratio):
    RATIOS[lab] = max(RATIOS.get(lab, 0.0), ratio)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    lines = [f"{r:8.4f}  {lab}" for lab, r in sorted(RATIOS.items())]
    print("\nworst err / bound per kernel label\n" + "\n".join(lines))
    path = os.environ.get("SRGANFD_CONV_PATHS_REPORT")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


_REF = {}              # (case, dtype, cin, dims) -> host data and the float64 reference, computed once for the NHWC and the planar run


def _reference(case, dtype, cin, dims):
    key = (case["name"], dtype, cin, dims)
    if key in _REF:
        return _REF[key]
    _REF.clear()                                              # one entry: the planar run follows the NHWC run of the same case
    n, hi, wi, ho, wo, cout = dims
    cs = case["cout_store"] or cout
    g = torch.Generator().manual_seed(1234 + cin + 7 * len(case["name"]))
    rnd = lambda *s: torch.randn(*s, generator=g)
    D = {"x": (rnd(n, hi, wi, cin) * 0.7).to(dtype)}
    for nm in ("r1", "r2", "mask"):
        if case[nm] is not None:
            D[nm] = rnd(n, ho, wo, cs).to(dtype)
    D["bias"] = rnd(cs) if case["bias"] else None
    D["alpha_dev"] = torch.tensor([case["alpha_dev"]], dtype=F32) if case["alpha_dev"] else None
    kw = dict(alpha=f32r(case["alpha"]), alpha_dev=D["alpha_dev"], bias=D["bias"], act=case["act"], slope=f32r(case["slope"]),
              post_scale=f32r(case["post_scale"]), r1=D.get("r1"), r1_scale=f32r(case["r1"] or 0), r2=D.get("r2"), r2_scale=f32r(case["r2"] or 0),
              mask=D.get("mask"), mask_slope=f32r(case["mask"] or 0))
    if case["form"]:
        kf, _, kc, _, _, _ = O.CLASS_FORMS[case["form"]]
        D["wt"] = rnd(cin, cout, kf, kf) / (cin * kc * kc) ** 0.5                 # the stride-2 conv's weight: (co, ci) = (cin of the gradient pass, cout)
        D["K"] = kc * kc * cin
        ws = [O.weight_class(D["wt"].to(dtype), case["form"], par) for par in range(4)]
        D["ref"] = O.conv2d_classes(D["x"], ws, case["form"], **kw)
    else:
        k = case["k"]
        D["K"] = k * k * cin
        if case["transposed"]:
            D["wt"] = rnd(cin, cs, k, k) / (cin * k * k) ** 0.5
            wl = O.weight_dgrad(D["wt"].to(dtype))
        else:
            D["wt"] = rnd(cs, cin, k, k) / (cin * k * k) ** 0.5
            wl = D["wt"].to(dtype)
        D["ref"] = O.conv2d(D["x"], wl, stride=case["s"], pad=case["p"], up=case["up"], **kw)
    assert D["ref"][0].shape == (n, ho, wo, cs)
    _REF[key] = D
    return D


def _pack(case, dtype, cin, cout, wt):
    """(packed operand(s) on the device, bytes per operand)"""
    from sr_gan_fd_amd import ops
    dt = ops.DT[dtype]
    if not case["form"]:
        return ops.pack_single(wt.cuda(), dt, transposed=case["transposed"]), 0
    _, _, kc, code, _, _ = O.CLASS_FORMS[case["form"]]
    pb = ops.packed_bytes(dt, kc, cin, cout)
    packed = torch.empty(4 * pb, dtype=torch.uint8, device="cuda")
    jobs = [ops.pack_job(c * pb, dt, kc, cin, cout, [dict(src_off=0, co_src=cin, ci_src=cout, k_len=cin, transposed=code + c)]) for c in range(4)]
    ops.PackTable(jobs, torch.device("cuda")).run(wt.cuda().contiguous(), packed)
    return packed, pb


def _run(case, dtype, cin, planar, dims, tag=""):
    from sr_gan_fd_amd import _abi as A, ops, profiling
    n, hi, wi, ho, wo, cout = dims
    D = _reference(case, dtype, cin, dims)
    L = layout(case, dtype, cin, planar, dims)
    what = f"{case['name']} {NAME[dtype]} cin {cin} {'planar' if planar else 'nhwc'}"
    g = torch.Generator().manual_seed(99)
    ins = {}
    for nm in ("x", "r1", "r2", "mask"):
        if nm in L:
            h, w, cbuf, c0, c, pl, et = L[nm]
            # the shared buffer: the sentinel (not zero) everywhere but the input channels, the output slice included
            ins[nm] = O.Buf(n, h, w, cbuf, et, pl, fill="sentinel" if case.get("shared") else "garbage", gen=g)
            ins[nm].put(c0, D[nm])
            ins[nm].upload()
    packed, pb = _pack(case, dtype, cin, cout, D["wt"])
    bias = D["bias"].cuda() if D["bias"] is not None else None
    adev = D["alpha_dev"].cuda() if D["alpha_dev"] is not None else None

    def outputs():
        outs = {}
        for nm in ("y", "y2"):
            if nm in L:
                h, w, cbuf, c0, c, pl, et = L[nm]
                outs[nm] = ins["x"] if case.get("shared") else O.Buf(n, h, w, cbuf, et, pl).upload()
        return outs

    def check(outs, lab, par):
        torch.cuda.synchronize()
        worst = 0.0
        for nm, ref in (("y", D["ref"][0]), ("y2", D["ref"][1])):
            if nm not in outs:
                continue
            h, w, cbuf, c0, c, pl, et = L[nm]
            got = outs[nm].download()
            pix = None if par in (None, 4) else (par >> 1, 2, par & 1, 2)
            outs[nm].assert_outside_untouched(got, c0, c, f"{what} {nm}", pix)
            val, want, mag = got[..., c0:c0 + c], ref, D["ref"][2]
            if pix is not None:
                val, want, mag = (t[:, pix[0]::2, pix[2]::2] for t in (val, want, mag))
            ratio, at = O.worst_ratio(val, want, mag, D["K"], et)
            print(f"{what} {nm}{'' if par is None else f' class {par}'}: worst err / bound {ratio:.4f}  [{lab}]")
            assert ratio <= 1.0, f"{what} {nm}: element {at} is {ratio:.3f} times its bound ({lab})"
            worst = max(worst, ratio)
        _record(lab + tag, worst)

    first = outputs()
    views = {nm: b.view(A, L[nm][3]) for nm, b in {**ins, **first}.items()}
    for i, (a, lab, par) in enumerate(launches(case, dtype, cin, dims, views, packed.data_ptr(), pb, bias, adev)):
        outs = outputs() if i else first                  # every class launch writes a fresh sentinel buffer
        a.y = outs["y"].view(A, L["y"][3])
        assert profiling.conv_label(a) == lab, f"{what}: {profiling.conv_label(a)}, expected {lab}"
        ops.conv2d(a)
        check(outs, lab, par)                             # (the shared buffer: its input channels lie outside y's slice, so they are held too)


@pytest.mark.gpu
@pytest.mark.parametrize("p", SMALL_PARAMS, ids=[small_id(p) for p in SMALL_PARAMS])
def test_small_shapes_every_instantiation_and_operand(p):
    case, dtype, cin, planar = p
    _run(case, dtype, cin, planar, geometry(case, dtype, cin))


@pytest.mark.gpu
@pytest.mark.parametrize("p", PERSISTENT_PARAMS, ids=[f"{c['name']}-{NAME[dt]}-{'planar' if pl else 'nhwc'}" for c, dt, pl in PERSISTENT_PARAMS])
def test_persistent_tiles(p):
    """workgroups that run three tiles and workgroups that run two, by the host's own rule for this device's compute units (the cases
    of kinds 1 / 3 / 4: that many tiles, one per workgroup, unless the library was built with -DSRGANFD_CROSS_MASK=0)"""
    case, dtype, planar = p
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n, nblk, grid = persistent_batch(case, cus)
    assert nblk > 2 * cus, "not a persistent launch on this device"
    assert nblk > 2 * grid, "no workgroup runs a third tile"
    assert nblk % grid != 0, "every workgroup runs the same number of tiles"
    assert nblk % 8 != 0, "the even arm of xcd_remap only"
    if case.get("changes_block"):
        assert block_changes(case, nblk, grid), "every workgroup keeps one channel block: a stale weight block or bias would not show"
    _run(case, dtype, case["cin"], planar, (n, PH, PW, PH, PW, case["cout"]), tag=" @ 2.4 grids of tiles")
