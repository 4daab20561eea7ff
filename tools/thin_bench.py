"""Time the thin-side kernels (csrc/conv_thin.hip), by default beside the 32-channel-padded conv_igemm / wgrad launches they replace.

    python tools/thin_bench.py [--only-thin] [--n 32] [--h 512] [--w 512] [--dtype f16|bf16] [--iters 20]

One line per launch kind and thin channel count (3 and 1): microseconds per launch and the bandwidth over the bytes the launch must move.
The sizes also come from the environment (TB_N, TB_H, TB_W), which is how the A/B scripts pass them.  At the default 32 x 512 x 512
thin_in's outputs are large enough for its non-temporal instantiation; --only-thin skips the padded comparisons (and their buffers)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from sr_gan_fd_amd import _abi as A, ops


def timeit(fn, n):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only-thin", action="store_true")
    ap.add_argument("--n", type=int, default=int(os.environ.get("TB_N", 32)))
    ap.add_argument("--h", type=int, default=int(os.environ.get("TB_H", 512)))
    ap.add_argument("--w", type=int, default=int(os.environ.get("TB_W", 512)))
    ap.add_argument("--dtype", choices=("f16", "bf16"), default="f16")
    ap.add_argument("--iters", type=int, default=20)
    o = ap.parse_args()
    N, H, W = o.n, o.h, o.w
    dt, dtc = (torch.float16, A.F16) if o.dtype == "f16" else (torch.bfloat16, A.BF16)
    big = torch.randn(N, H, W, 64, device="cuda").to(dt)
    act = torch.randn(N, H, W, 64, device="cuda").to(dt)
    thin = torch.zeros(N, H, W, 4, dtype=dt, device="cuda")
    thin[..., :3] = torch.randn(N, H, W, 3, device="cuda").to(dt)
    y = torch.empty(N, H, W, 64, dtype=dt, device="cuda")
    o4 = torch.empty(N, H, W, 4, dtype=torch.float32, device="cuda")
    ws = torch.empty(ops.thin_wgrad_workspace_bytes(), dtype=torch.uint8, device="cuda")
    px = N * H * W
    for cs in (3, 1):
        Win = torch.randn(64, cs, 3, 3, device="cuda") * 0.1
        Wout = torch.randn(cs, 64, 3, 3, device="cuda") * 0.1
        b64, bcs = torch.randn(64, device="cuda"), torch.randn(cs, device="cuda")
        a_in = ops.thin_args(dtc, N, H, W, cs, Win, A.view(y), w_big_is_cout=True, bias=b64, act=A.ACT_LRELU, thin=thin)
        a_inm = ops.thin_args(dtc, N, H, W, cs, Wout, A.view(y), w_big_is_cout=False, flip=True, mask=A.view(act), thin=thin)
        a_out = ops.thin_args(dtc, N, H, W, cs, Wout, A.view(big), w_big_is_cout=False, bias=bcs, thin_out=o4)
        a_wg1 = ops.thin_args(dtc, N, H, W, cs, Win, A.view(big), w_big_is_cout=True, thin=thin)
        a_wg0 = ops.thin_args(dtc, N, H, W, cs, Wout, A.view(big), w_big_is_cout=False, thin=thin)
        dw1, db1 = torch.empty_like(Win), torch.empty(64, device="cuda")
        dw0, db0 = torch.empty_like(Wout), torch.empty(cs, device="cuda")
        res = {
            "thin_in": (timeit(lambda: ops.thin_in(a_in), o.iters), px * (8 + 128)),
            "thin_in+mask": (timeit(lambda: ops.thin_in(a_inm), o.iters), px * (8 + 256)),
            "thin_out": (timeit(lambda: ops.thin_out(a_out), o.iters), px * (128 + 16)),
            "thin_wgrad(big=dy)": (timeit(lambda: ops.thin_wgrad(a_wg1, dw1, db1, ws), o.iters), px * (128 + 8)),
            "thin_wgrad(big=x)": (timeit(lambda: ops.thin_wgrad(a_wg0, dw0, db0, ws), o.iters), px * (128 + 8)),
        }
        if not o.only_thin:           # the padded launches they replace
            pad32 = torch.zeros(N, H, W, 32, dtype=dt, device="cuda")
            pad32[..., :3] = thin[..., :3]
            c_in = ops.conv_args(dtc, A.view(pad32), A.view(y), ops.pack_single(Win, dtc), N, H, W, 32, 64, bias=b64, act=A.ACT_LRELU)
            c_inm = ops.conv_args(dtc, A.view(pad32), A.view(y), ops.pack_single(Wout, dtc, transposed=True), N, H, W, 32, 64, mask=A.view(act), mask_slope=0.2)
            c_out = ops.conv_args(dtc, A.view(big), A.view(o4), ops.pack_single(Wout, dtc), N, H, W, 64, 32, cout_store=cs, bias=bcs, y_f32=True)
            res["padded 32->64"] = (timeit(lambda: ops.conv2d(c_in), o.iters), px * (64 + 128))
            res["padded 32->64+mask"] = (timeit(lambda: ops.conv2d(c_inm), o.iters), px * (64 + 256))
            res["padded 64->%d" % cs] = (timeit(lambda: ops.conv2d(c_out), o.iters), px * (128 + 16))
            g = torch.empty(64 * 32 * 9 + 64, device="cuda")
            p1 = ops.WgradPlan("cuda", dtc, N, H, W, 32, 64, [dict(cin=32, cout=64, dw_off=0, db_off=64 * cs * 9, co_dst=64, ci_dst=cs)])
            wsb = torch.empty(p1.workspace_bytes, dtype=torch.uint8, device="cuda")
            res["padded wgrad %d->64" % cs] = (timeit(lambda: p1.run(A.view(pad32), A.view(big), g, wsb), o.iters), px * (64 + 128))
            p0 = ops.WgradPlan("cuda", dtc, N, H, W, 64, 32, [dict(cin=64, cout=32, dw_off=0, db_off=64 * cs * 9, co_dst=cs, ci_dst=64)])
            wsb0 = torch.empty(p0.workspace_bytes, dtype=torch.uint8, device="cuda")
            res["padded wgrad 64->%d" % cs] = (timeit(lambda: p0.run(A.view(big), A.view(pad32), g, wsb0), o.iters), px * (128 + 64))
        for k, (us, nb) in res.items():
            print("cs %d  %-22s %8.1f us  %7.1f GB/s  (%s N=%d %dx%d, %.0f MB to move)" % (cs, k, us, nb / us / 1e3, o.dtype, N, H, W, nb / 1e6))


if __name__ == "__main__":
    main()
