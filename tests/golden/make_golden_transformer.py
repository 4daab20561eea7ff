#!/usr/bin/env python3
"""Writes tests/golden/transformer.npz by IMPORTING the reference's A-ESRGAN/model.py (with the stubs make_golden.py uses), building
a small BSRGANtrans in float64 and ``.eval()`` mode, and capturing with hooks what its ``transformer_encoder`` sees: the input, the
output, the gradients at both, the encoder's state and its parameter gradients.  The capture goes through the reference's own
forward text (model.py:725-727: ``permute(0, 2, 3, 1).flatten(1, 2)`` into a batch_first=False stack), which pins the orientation:
the sequence axis is the BATCH of images, every pixel position a sequence of its own.

Data only.  The encoder's parameters are put on the float16 grid before the run and stored in that type; inputs, outputs and
gradients are float64; a parameter gradient of more than 4096 elements (linear1 / linear2 weights at the reference's hidden size of
2048) is stored as make_golden.checksum's three sums.  Also stored: keys, shapes and checksums of the encoder's state after a
``torch.manual_seed(0)`` construction of ``TransformerEncoder(TransformerEncoderLayer(64, 4), 2)`` as the reference spells it.

    python tests/golden/make_golden_transformer.py        (SRGAN_REFERENCE names the reference tree)
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import checksum, load_ref  # noqa: E402

CHANNELS, GROWTH, RRDB, BATCH, LR_H, LR_W = 8, 4, 1, 3, 6, 8
BIG = 4096


def main():
    warnings.simplefilter("ignore")
    ref = load_ref("A-ESRGAN")
    out = {}
    torch.manual_seed(5)
    net = ref.BSRGANtrans(channels=CHANNELS, growth_channels=GROWTH, num_rrdb=RRDB, upscale_factor=2).double().eval()
    enc = net.transformer_encoder
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 4:
                p.mul_(10.0)                            # the reference's 0.1-scaled init leaves the encoder's input near zero
        for p in enc.parameters():
            p.copy_(p.to(torch.float16).double())
    cap = {}
    enc.register_forward_hook(lambda m, i, o: cap.update(src=i[0].detach().clone(), out=o.detach().clone()))
    enc.register_full_backward_hook(lambda m, gi, go: cap.update(dsrc=gi[0].detach().clone(), dout=go[0].detach().clone()))
    g = torch.Generator().manual_seed(6)
    x = torch.rand(BATCH, 3, LR_H, LR_W, generator=g, dtype=torch.float64)
    sr = net(x)
    (sr * torch.randn(sr.shape, generator=g, dtype=torch.float64)).sum().backward()
    S, N, E = cap["src"].shape
    assert (S, N, E) == (BATCH, (LR_H // 2) * (LR_W // 2), CHANNELS), cap["src"].shape
    assert net.transformer_layer.linear1.weight.grad is None          # the registered copy the forward never calls
    for k in ("src", "out", "dsrc", "dout"):
        out[k] = cap[k].numpy()
    out["orientation"] = np.array([S, N, E, BATCH, LR_H // 2, LR_W // 2], dtype=np.int64)      # (S, N, E) and the (B, h, w) it came from
    out["nhead"] = np.array(enc.layers[0].self_attn.num_heads, dtype=np.int64)
    for k, v in enc.state_dict().items():
        out["state." + k] = v.numpy().astype(np.float16)
        assert np.array_equal(out["state." + k].astype(np.float64), v.numpy()), k
    for k, p in enc.named_parameters():
        out[("gradsum." if p.numel() > BIG else "grad.") + k] = checksum(p.grad) if p.numel() > BIG else p.grad.numpy()
    # a seeded construction as the reference spells it: keys, shapes, checksums
    torch.manual_seed(0)
    layer = ref.TransformerEncoderLayer(d_model=64, nhead=4)
    seeded = ref.TransformerEncoder(layer, num_layers=2)
    out["seeded.keys"] = np.array(list(seeded.state_dict()))
    for k, v in seeded.state_dict().items():
        out["seeded.shape." + k] = np.array(v.shape, dtype=np.int64)
        out["seeded.sum." + k] = checksum(v)
    path = os.path.join(HERE, "transformer.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; src", tuple(cap["src"].shape), "|src| max %.3f" % float(cap["src"].abs().max()))


if __name__ == "__main__":
    main()
