#!/usr/bin/env python3
"""Writes tests/golden/attention.npz by IMPORTING the reference's BSRGAN/model.py (with the stubs make_golden.py uses) and running
its SelfAttention in float64 on cases A and C of tests/attention_oracle.py.  Data only: per case the input, the state dict and the
reference's two outputs.  Inputs and parameters lie on the float16 grid (attention_oracle.make_case) and are stored in that type;
the outputs are float64.

    python tests/golden/make_golden_attention.py        (SRGAN_REFERENCE names the reference tree)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import attention_oracle as AO  # noqa: E402
from make_golden import load_ref  # noqa: E402

FIXTURE_CASES = ("A", "C")


def main():
    ref = load_ref("BSRGAN")
    out = {}
    for name in FIXTURE_CASES:
        c, heads, x, state, _ = AO.case_inputs(name)
        m = ref.SelfAttention(c, heads).double()
        m.load_state_dict({k: v.double() for k, v in state.items()})
        with torch.no_grad():
            y, wts = m(x.double())
        peak = AO.peakedness(wts)
        assert peak >= 3.0, (name, peak)
        out[name + ".x"] = x.numpy().astype(np.float16)
        assert np.array_equal(out[name + ".x"].astype(np.float32), x.numpy())
        for k, v in state.items():
            out[name + ".state." + k] = v.numpy().astype(np.float16)
            assert np.array_equal(out[name + ".state." + k].astype(np.float32), v.numpy())
        out[name + ".out"], out[name + ".weights"] = y.numpy(), wts.numpy()
        print(name, tuple(x.shape), "peakedness %.2f x 1/L" % peak)
    path = os.path.join(HERE, "attention.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
