#!/usr/bin/env python3
"""Writes tests/golden/rpa.npz by IMPORTING the reference's A-ESRGAN/model.py (with the stubs make_golden.py uses) and running its
RPA, US and Generator_RPA in float64 on rpa_oracle.FIXTURE_CASES (num_feat 4: about 130 KB, most of it the float64 gradients).  Data only:
  <case>.x, <case>.state.<key>, <case>.d_out      inputs, on the float16 grid and stored in that type
  <case>.out, <case>.dx, <case>.grad.<key>        the reference's float64 output, input gradient and parameter gradients
  <case>.sigmoid_q                                5 % and 95 % quantile of every sigmoid the case evaluates
  init.<Class>.keys / .shapes / .checksums        ordered state-dict keys, their shapes (padded to 4) and tests.util.checksum of every
                                                  tensor of a torch.manual_seed(0) construction of RPA(64), US(64, 2) and
                                                  Generator_RPA(scale=2, num_block=2)

    python tests/golden/make_golden_rpa.py        (SRGAN_REFERENCE names the reference tree)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import rpa_oracle as RO  # noqa: E402
from make_golden import checksum, load_ref  # noqa: E402


def build(ref, kind, nf, nb, scale):
    if kind == "rpa":
        return ref.RPA(nf)
    if kind == "us":
        return ref.US(nf, 2)
    return ref.Generator_RPA(scale=scale, num_feat=nf, num_block=nb)


def main():
    ref = load_ref("A-ESRGAN")
    out = {}
    for name, (kind, shape, nf, nb, scale, seed) in RO.FIXTURE_CASES.items():
        x, state, d_out = RO.make_case(kind, shape, seed, nf, nb, scale)
        m = build(ref, kind, nf, nb, scale).double()
        assert list(m.state_dict()) == list(state), name
        m.load_state_dict({k: v.double() for k, v in state.items()})
        sig = []
        hooks = [mod.register_forward_hook(lambda _m, _i, o: sig.append(o.detach().flatten())) for mod in m.modules() if isinstance(mod, torch.nn.Sigmoid)]
        xl = x.double().requires_grad_(True)
        y = m(xl)
        y.backward(d_out.double())
        for h in hooks:
            h.remove()
        q = torch.quantile(torch.cat(sig), torch.tensor([0.05, 0.95], dtype=torch.float64))
        assert q[0] < 0.2 and q[1] > 0.8, (name, q)
        for key, t in [("x", x), ("d_out", d_out)] + [("state." + k, v) for k, v in state.items()]:
            out[f"{name}.{key}"] = t.numpy().astype(np.float16)
            assert np.array_equal(out[f"{name}.{key}"].astype(np.float32), t.numpy()), key
        out[name + ".out"], out[name + ".dx"], out[name + ".sigmoid_q"] = y.detach().numpy(), xl.grad.numpy(), q.numpy()
        for k, p in m.named_parameters():
            out[f"{name}.grad.{k}"] = p.grad.numpy()
        print(name, tuple(x.shape), "->", tuple(y.shape), "sigmoid quantiles %.3f / %.3f" % (q[0], q[1]))
    for cls, make in (("RPA", lambda: ref.RPA(64)), ("US", lambda: ref.US(64, 2)), ("Generator_RPA", lambda: ref.Generator_RPA(scale=2, num_block=2))):
        torch.manual_seed(0)
        sd = make().state_dict()
        out[f"init.{cls}.keys"] = np.array(list(sd))
        out[f"init.{cls}.shapes"] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()], dtype=np.int64)
        out[f"init.{cls}.checksums"] = np.stack([checksum(v) for v in sd.values()])
    path = os.path.join(HERE, "rpa.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
