"""Reader of tests/golden/realesrgan_kernels.npz (tests/golden/make_golden_realesrgan_kernels.py: the filter kernels the reference's
Real-ESRGAN dataset makes on the host) and the bound its kernels are compared under.  numpy only."""
import json

import numpy as np


def load_fixture(path):
    """{"config": the degradation-model parameters, "sweep": [{"family", "kind", "ksize", "params" (5,), "ref" (k, k) float64}],
    "seeds": {seed: {"draws", "end" (2,), "gaussian_kernel1" / "gaussian_kernel2" / "sinc_kernel" (B, K, K) float32}}}"""
    z = np.load(path)
    sweep, at = [], 0
    for family, kind, k, params in zip(z["sweep_family"], z["sweep_kind"], z["sweep_ksize"], z["sweep_params"]):
        k = int(k)
        sweep.append({"family": str(family), "kind": int(kind), "ksize": k, "params": params, "ref": z["sweep_values"][at:at + k * k].reshape(k, k)})
        at += k * k
    assert at == z["sweep_values"].size
    seeds = {}
    for s in z["seeds"]:
        s = int(s)
        seeds[s] = {"draws": json.loads(str(z[f"seed{s}_draws"])), "end": z[f"seed{s}_end"]}
        for key in ("gaussian_kernel1", "gaussian_kernel2", "sinc_kernel"):
            seeds[s][key] = z[f"seed{s}_{key}"]
    return {"config": json.loads(str(z["config"])), "sweep": sweep, "seeds": seeds}


def centred(ref, kmax):
    """a k x k kernel in the middle of a kmax x kmax array of zeros"""
    k = ref.shape[0]
    out = np.zeros((kmax, kmax), dtype=ref.dtype)
    o = (kmax - k) // 2
    out[o:o + k, o:o + k] = ref
    return out


def compare(out, ref):
    """``out``: one float32 kernel; ``ref``: the reference's values for it, float64 or float32.  Returns (largest excess over the bound --
    <= 0 passes --, number of elements that are not bit-equal to float32(ref)).  The bound, with ref32 = float32(ref):
        |out - ref32| <= np.spacing(|ref32|) + 1e-12 max|ref|
    Both sides evaluate in fp64 and round once, so fp64 differences (another exp / pow / j1, another summation order over at most 441
    terms) can only move a value across one float32 rounding boundary; the absolute term covers J1 near its zeros and values in float32's
    subnormal range."""
    out = np.asarray(out)
    assert out.dtype == np.float32 and out.shape == ref.shape
    ref32 = np.asarray(ref, dtype=np.float32)
    allowed = np.spacing(np.abs(ref32)).astype(np.float64) + 1e-12 * np.abs(np.asarray(ref, dtype=np.float64)).max()
    err = np.abs(out.astype(np.float64) - ref32.astype(np.float64))
    return float((err - allowed).max()), int((out.view(np.uint32) != ref32.view(np.uint32)).sum())
