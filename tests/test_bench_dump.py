"""bench.py --dump-outputs on the host: which arrays a dump holds, their dtype, the 64 MB bound, and the seeded sample that stands
for an array larger than DUMP_MAX_ELEMS (the same positions in every run, drawn in order from the array)."""
import types

import numpy as np
import torch

import bench


def _trainer(n_params):
    g = torch.Generator().manual_seed(3)
    opt = types.SimpleNamespace(flat=torch.rand(n_params, generator=g), ema=torch.rand(n_params, generator=g))
    return types.SimpleNamespace(opt=opt, sr=torch.rand(2, 3, 8, 8, generator=g))


def test_dump_holds_the_step_output_sr_weights_and_ema(tmp_path):
    tr = _trainer(1000)
    bench.dump_outputs(str(tmp_path), torch.tensor([0.25]), tr, None)
    names = sorted(p.name for p in tmp_path.iterdir())
    assert names == ["g_ema.npy", "g_params.npy", "sr.npy", "step_output.npy"]
    assert np.array_equal(np.load(tmp_path / "sr.npy"), tr.sr.numpy())
    assert np.array_equal(np.load(tmp_path / "g_params.npy"), tr.opt.flat.numpy())
    assert np.array_equal(np.load(tmp_path / "g_ema.npy"), tr.opt.ema.numpy())
    assert np.load(tmp_path / "step_output.npy").dtype == np.float32


def test_large_arrays_are_a_fixed_seeded_sample(tmp_path):
    n = bench.DUMP_MAX_ELEMS + 12345
    tr = _trainer(n)
    tr.opt.flat = torch.arange(n, dtype=torch.float64)      # value == position: the sample shows where it was drawn
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), torch.tensor([1.0]), tr, None)
    p = np.load(tmp_path / "a" / "g_params.npy")
    assert p.dtype == np.float64 and p.shape == (bench.DUMP_MAX_ELEMS,)
    assert np.all(np.diff(p) >= 0) and p[0] >= 0 and p[-1] < n and len(np.unique(p)) > bench.DUMP_MAX_ELEMS // 2
    for name in ("g_params.npy", "g_ema.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name))
    e = np.load(tmp_path / "a" / "g_ema.npy")
    assert e.dtype == np.float32 and e.shape == (bench.DUMP_MAX_ELEMS,)
    assert sum((tmp_path / "a" / f).stat().st_size for f in ("g_params.npy", "g_ema.npy", "sr.npy", "step_output.npy")) <= 64 << 20
