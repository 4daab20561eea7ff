#!/usr/bin/env python3
"""What Real-ESRGAN's filter-kernel synthesis costs on the device, at the training shape (batch 48, 3x256x256 GT, three kernels per image,
kmax 21: realesrgan_config.py:46-65, :116-117; the parameter dict is read from tests/golden/realesrgan_kernels.npz).

    python tools/kernel_bank_bench.py [--batch 48] [--size 256] [--iters 20] [--out profiles/kernel_bank_bench.txt]

One JSON line per item, printed and written to --out:
  * srganfd_blur_kernel_bank alone: one launch for the 3 x batch kernels of a seeded draw, arguments already on the device; HIP events
    around --bank-iters launches after a warm-up.  Beside it, what a caller of imgproc pays per batch: realesrgan_kernel_draws on the host
    (host clock) and realesrgan_blur_kernels with its three small uploads (host clock around a device synchronise).
  * imgproc.degradation_process fed the bank's per-image kernels, beside the one fixed random 21 x 21 kernel tools/degrade_bench.py
    passes three times: the same seeded branches for both, alternated over --rounds rounds, HIP events; per-round times and the medians.
  * the share of the fixture's sweep elements (tests/golden/realesrgan_kernels.npz) whose bits differ from float32(reference).
There is no pass threshold.  Needs a GPU: without one it fails."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tools.degrade_bench import PARAMS, timed  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "realesrgan_kernels.npz")


def kernel_params():
    """the degradation-model parameters of the reference's config, as the tests' fixture records them"""
    return json.loads(str(np.load(FIXTURE)["config"]))


def seed_all(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--bank-iters", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "kernel_bank_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kernel_bank_bench: needs a GPU")
    from sr_gan_fd_amd import _abi as A, imgproc
    b, n = a.batch, a.size
    KERNEL_PARAMS = kernel_params()
    lines = []

    def out(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    out({"device": torch.cuda.get_device_name(0), "batch": b, "gt": f"3x{n}x{n}", "kernels per bank": 3 * b, "kmax": 21})
    # ---- the bank alone
    seed_all(0)
    draws = imgproc.realesrgan_kernel_draws(b, KERNEL_PARAMS)
    recs = [rec[name] for name in ("kernel1", "kernel2", "sinc_kernel") for rec in draws]
    kind = torch.tensor([r["kind"] for r in recs], dtype=torch.int32, device="cuda")
    ksize = torch.tensor([r["ksize"] for r in recs], dtype=torch.int32, device="cuda")
    params = torch.tensor([[r[f] for f in ("sigma_x", "sigma_y", "theta", "beta", "omega")] for r in recs], dtype=torch.float64, device="cuda")
    bank = torch.empty(3 * b, 21, 21, device="cuda")
    L = A.lib()

    def launch():
        A.check(L.srganfd_blur_kernel_bank(kind.data_ptr(), ksize.data_ptr(), params.data_ptr(), None, None, 3 * b, 21, bank.data_ptr(), A.stream_ptr()),
                "blur_kernel_bank")
    t_bank = [timed(launch, a.bank_iters) for _ in range(a.rounds)]
    t0 = time.perf_counter()
    for _ in range(a.iters):
        imgproc.realesrgan_kernel_draws(b, KERNEL_PARAMS)
    t_draws = (time.perf_counter() - t0) / a.iters
    for _ in range(3):
        imgproc.realesrgan_blur_kernels(draws, KERNEL_PARAMS)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        imgproc.realesrgan_blur_kernels(draws, KERNEL_PARAMS)
    torch.cuda.synchronize()
    t_wrap = (time.perf_counter() - t0) / a.iters
    kinds = [int((kind == k).sum()) for k in range(5)]
    out({"stage": f"srganfd_blur_kernel_bank, {3 * b} kernels in one launch (HIP events, {a.bank_iters} back-to-back launches per round)",
         "us per launch, rounds": [round(t * 1e6, 2) for t in t_bank], "us per launch, median": round(statistics.median(t_bank) * 1e6, 2),
         "kinds (delta, gaussian, generalized, plateau, sinc)": kinds})
    out({"stage": "per batch on the host side of the package (host clock)", "realesrgan_kernel_draws us": round(t_draws * 1e6, 1),
         "realesrgan_blur_kernels (3 uploads + launch, then synchronise) us": round(t_wrap * 1e6, 1)})
    # ---- degradation_process with per-image kernels against the fixed kernel of tools/degrade_bench.py
    k1, k2, sinc = imgproc.realesrgan_blur_kernels(draws, KERNEL_PARAMS)
    seed_all(0)
    gt = torch.rand(b, 3, n, n, device="cuda")
    k21 = torch.rand(b, 21, 21, device="cuda")
    k21 = k21 / k21.sum(dim=(1, 2), keepdim=True)
    usm, jpeg = imgproc.USMSharp().cuda(), imgproc.DiffJPEG().cuda()
    t_fixed, t_bank_fed = [], []
    for _ in range(a.rounds):
        for ks, acc in (((k21, k21, k21), t_fixed), ((k1, k2, sinc), t_bank_fed)):
            seed_all(0)                                   # the same random branches for both, every round
            acc.append(timed(lambda: imgproc.degradation_process(gt, ks[0], ks[1], ks[2], 4, PARAMS, jpeg, usm), a.iters))
    out({"stage": "degradation_process (USM + 2nd-order pipeline, the same seeded branches), HIP events", "iters per round": a.iters,
         "fixed random k21 x 3, ms per round": [round(t * 1e3, 3) for t in t_fixed], "bank's per-image kernels, ms per round": [round(t * 1e3, 3) for t in t_bank_fed],
         "fixed ms, median": round(statistics.median(t_fixed) * 1e3, 3), "bank-fed ms, median": round(statistics.median(t_bank_fed) * 1e3, 3)})
    # ---- the share of elements that are not bit-equal to float32(reference), over the fixture's sweep (reported; the tests hold the bound)
    from tests import realesrgan_kernels_oracle as KO
    sweep = KO.load_fixture(FIXTURE)["sweep"]
    got = imgproc.blur_kernel_bank([c["kind"] for c in sweep], [c["ksize"] for c in sweep], np.stack([c["params"] for c in sweep]), 21).cpu().numpy()
    results = [KO.compare(got[i], KO.centred(c["ref"], 21)) for i, c in enumerate(sweep)]
    unequal, total = sum(r[1] for r in results), sum(c["ksize"] ** 2 for c in sweep)
    out({"stage": f"the fixture's {len(sweep)} sweep kernels in one launch against float32(reference)", "elements": total, "not bit-equal": unequal,
         "share not bit-equal": unequal / total, "inside the bound |out - ref32| <= spacing(|ref32|) + 1e-12 max|ref|": all(r[0] <= 0 for r in results)})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
