#!/usr/bin/env python3
"""Writes tests/golden/bsrgantrans.npz by IMPORTING the reference's A-ESRGAN/model.py (with the stubs make_golden.py uses): what its
own ``BSRGANtrans`` computes, forward and backward, for one small batch.  Data only.

Recipe (tests/bsrgantrans_oracle.edit repeats the three edits on this repository's seeded module):
``torch.manual_seed(5)``, ``BSRGANtrans(channels=64, growth_channels=32, num_rrdb=1, upscale_factor=2)`` (nhead = 4 is hard-coded in
the reference: 64 is the smallest width with an attention kernel); every 4-D parameter times 8 and ``conv4.bias`` = 0.5 (the stock
0.1-scaled initialisation gives an SR of standard deviation 4e-5, half of it clamped); the parameters of ``transformer_encoder`` rounded
to the float16 grid; float64, ``.eval()``.  Input ``torch.rand(3, 3, 6, 8)``, the SR's gradient a seeded normal.

Stored: input, SR, the SR's gradient, the input's gradient; the encoder's captured input and output; every parameter's gradient
(make_golden.checksum's three sums for anything over 4096 elements); the names of the parameters whose gradient is None
(``transformer_layer.*``: registered, never called); and ``seeded.*``: keys, shapes and checksums of the state dict right after the
seeded construction, before the edits -- the 1.75 M parameters themselves are not stored.

    python tests/golden/make_golden_bsrgantrans.py        (SRGAN_REFERENCE names the reference tree)
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import checksum, load_ref  # noqa: E402

CHANNELS, GROWTH, RRDB, BATCH, LR_H, LR_W = 64, 32, 1, 3, 6, 8
SEED, SCALE, BIAS, BIG = 5, 8.0, 0.5, 4096


def main():
    warnings.simplefilter("ignore")
    ref = load_ref("A-ESRGAN")
    out = {}
    torch.manual_seed(SEED)
    net = ref.BSRGANtrans(channels=CHANNELS, growth_channels=GROWTH, num_rrdb=RRDB, upscale_factor=2)
    out["seeded.keys"] = np.array(list(net.state_dict()))
    for k, v in net.state_dict().items():
        out["seeded.shape." + k] = np.array(v.shape, dtype=np.int64)
        out["seeded.sum." + k] = checksum(v)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 4:
                p.mul_(SCALE)
        net.conv4.bias.fill_(BIAS)
        for p in net.transformer_encoder.parameters():
            p.copy_(p.to(torch.float16).float())
    net = net.double().eval()
    cap = {}
    net.transformer_encoder.register_forward_hook(lambda m, i, o: cap.update(src=i[0].detach().clone(), out=o.detach().clone()))
    g = torch.Generator().manual_seed(SEED + 1)
    x = torch.rand(BATCH, 3, LR_H, LR_W, generator=g, dtype=torch.float64).requires_grad_(True)
    sr = net(x)
    dsr = torch.randn(sr.shape, generator=g, dtype=torch.float64)
    sr.backward(dsr)
    assert cap["src"].shape == (BATCH, (LR_H // 2) * (LR_W // 2), CHANNELS)
    out.update(x=x.detach().numpy(), sr=sr.detach().numpy(), dsr=dsr.numpy(), dx=x.grad.numpy(), enc_src=cap["src"].numpy(), enc_out=cap["out"].numpy())
    none = []
    for k, p in net.named_parameters():
        if p.grad is None:
            none.append(k)
        elif p.numel() > BIG:
            out["gradsum." + k] = checksum(p.grad)
        else:
            out["grad." + k] = p.grad.numpy()
    assert none and all(k.startswith("transformer_layer.") for k in none), none
    out["grad_none"] = np.array(none)
    clamped = float(((sr == 0) | (sr == 1)).double().mean())
    out["clamped_share"] = np.array(clamped)
    path = os.path.join(HERE, "bsrgantrans.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; clamped share %.3f, |enc_src| max %.3f" % (clamped, float(cap["src"].abs().max())))


if __name__ == "__main__":
    main()
