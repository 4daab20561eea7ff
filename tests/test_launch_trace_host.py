"""Every call the engines and fused trainers make into libsrganfd_hip.so, compared with a recorded trace.

In dry-run mode (``_abi.set_dry_run(True)``) the engines run on CPU tensors: every C entry point validates its arguments and
launches nothing, and every call goes through ``_abi.lib()``.  For the length of a scenario ``_abi._lib`` is a proxy that records
each call -- the entry point's name and every argument, structures expanded field by field -- and the record is compared with
tests/golden/launch_trace.json.gz.  The GPU tests compare numbers for a handful of shapes and the other host tests look at the
shapes of plans; this one sees which packed operand, which bias, which 1/sigma slot and which gradient offset every launch gets,
in which order, for all three GAN trainers, the generator trainer and the module paths through autograd.

What is recorded for a pointer (arguments and fields whose ctypes type is ``c_void_p``): null, or, when it points into one of the
long-lived buffers of an engine alive at the time of the call (``eng.fp.flat`` and, per ``eng.packed[dtype]``: ``buf``,
``scalars``, ``sn_ws``), ``"<EngineClass>[<parameter count>].<buffer>+<byte offset>"``, else ``"p"``.  Activation buffers and
per-call temporaries are ``"p"``: the allocator hands their addresses out differently from process to process.  Per engine and
dtype the scenario also records the hash of the pack table's bytes and the offsets of the packed operands.

Calls that enqueue work are compared in order.  Calls that only ask the library something while a plan is built (QUERIES) are
compared as a multiset per scenario, so building two plans in another order is not a failure.

The fixture is regenerated (``python tests/golden/make_golden_launch_trace.py``) only by a change that MEANS to change what is
launched -- a new kernel, another packing, a reordered schedule.  The difference in the fixture is then part of that change and
is to be reviewed like the code (decompress both versions and diff them: one call per line); a refactoring of the host code
leaves the fixture alone and this test passing.

The profiled path: with ``profiling.REC`` set, every conv, thin, dense-chain and weight-gradient launch goes through
``rec.bracket(label, work, fn)`` instead, and bench.py builds its ``kernel_classes`` and ``roofline`` fields from those labels and
work figures.  Each scenario runs a second time under a recorder stub that notes ``(label, flop, bytes)`` and calls ``fn``: the
trace must be the same one (but for the ``srganfd_conv2d_describe`` calls that ask the library for the labels) and the brackets,
in order, must equal tests/golden/launch_labels.json.gz (``python tests/golden/make_golden_launch_labels.py``, regenerated under
the same rule as the trace).
"""
import ctypes as C
import gzip
import hashlib
import json
import os
from collections import Counter

import pytest
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_trace.json.gz")
LABELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_labels.json.gz")
NODES = ["features.2", "features.7", "features.16", "features.25", "features.34"]
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
DTYPES = {"f32": torch.float32, "f16": torch.float16}
UNRECORDED = ("srganfd_last_error", "srganfd_set_dry_run", "srganfd_abi_version")
QUERIES = ("srganfd_pack_layout", "srganfd_wgrad_plan_bytes", "srganfd_wgrad_plan_build", "srganfd_dense_chain_check")


def is_query(name):
    return name in QUERIES or "_workspace" in name


def _sha(raw):
    return hashlib.sha1(raw).hexdigest()[:12]


def _engine_buffers():
    """(address, bytes, name) of the long-lived buffers of every engine alive now"""
    from sr_gan_fd_amd import engine as E
    out = []
    for eng in list(E._ENGINES.values()):
        tag = "%s[%d]" % (type(eng).__name__, eng.fp.total)
        if eng.fp.flat is not None:
            out.append((eng.fp.flat.data_ptr(), eng.fp.flat.numel() * 4, tag + ".flat"))
        for dtc, pk in eng.packed.items():
            for k in ("buf", "scalars", "sn_ws"):
                t = pk.get(k)
                if t is not None:
                    out.append((t.data_ptr(), t.numel() * t.element_size(), "%s.pk%d.%s" % (tag, dtc, k)))
    return out


class Recorder:
    """stands in for the CDLL object: records every srganfd_* call, then makes it"""

    def __init__(self, lib):
        self._lib, self._wrapped = lib, {}
        self.launches, self.queries = [], []
        self._bufs = None

    def _ptr(self, v):
        if not v:
            return None
        if self._bufs is None:
            self._bufs = _engine_buffers()
        for base, nbytes, name in self._bufs:
            if base <= v < base + nbytes:
                return "%s+%d" % (name, v - base)
        return "p"

    def _canon(self, v, ctype=None):
        if hasattr(v, "_obj"):                               # byref()
            return self._canon(v._obj)
        if isinstance(v, C.Structure):
            return {n: self._canon(getattr(v, n), t) for n, t in v._fields_}
        if isinstance(v, C.Array):
            if v._type_ is C.c_char:
                return "bytes:" + _sha(v.raw)
            return [self._canon(x, v._type_) for x in v]
        if isinstance(v, C._SimpleCData):
            return self._canon(v.value, type(v))
        if ctype is C.c_void_p:
            return self._ptr(v)
        if isinstance(v, float):
            return round(v, 9)
        if v is None or isinstance(v, (bool, int)):
            return v
        raise TypeError("launch trace: argument of type %r" % type(v))

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("srganfd_") or name in UNRECORDED or not callable(fn):
            return fn
        w = self._wrapped.get(name)
        if w is None:
            types = fn.argtypes or []
            dest = self.queries if is_query(name) else self.launches

            def w(*args):
                self._bufs = None
                dest.append([name] + [self._canon(a, types[i] if i < len(types) else None) for i, a in enumerate(args)])
                return fn(*args)
            self._wrapped[name] = w
        return w

    def tables(self):
        """per engine alive and dtype: hash of the pack table, offsets of the packed operands, size of the packed buffer"""
        from sr_gan_fd_amd import engine as E
        out = []
        for eng in E._ENGINES.values():
            for dtc, pk in eng.packed.items():
                out.append(["%s[%d].pk%d" % (type(eng).__name__, eng.fp.total, dtc), _sha(pk["table"].dev.numpy().tobytes()),
                            sorted([repr(k), v] for k, v in pk["offs"].items()), pk["buf"].numel()])
        return sorted(out)


# ---- scenarios: tiny shapes, num_rrdb=1 generators but for generator_only_rrdb2; each returns what must stay alive until the tables are read ----
def _pin(dt, *modules):
    for m in modules:
        m.compute_dtype = dt
    return modules


def _unet():
    from sr_gan_fd_amd import model as M
    return M.discriminator_unet(in_channels=3, out_channels=1, channels=64)


def _gan(dt, dfac, generator_first=False, content=True, usm=True, **kw):
    from sr_gan_fd_amd import model as M
    from sr_gan_fd_amd.gan import GanTrainer
    g, d = _pin(dt, M.bsrgan_x4(num_rrdb=1), dfac())
    cl = _pin(dt, M.ContentLoss(NODES, MEAN, STD))[0] if content else None
    tr = GanTrainer(g, d, cl, generator_first=generator_first, **kw)
    for _ in range(2):                 # the second step sees cached plans and stale packs
        tr.step(torch.rand(2, 3, 16, 16), torch.rand(2, 3, 64, 64), torch.rand(2, 3, 64, 64) if generator_first and usm else None)
    return g, d, cl, tr


def _esrgan(dt, content=True, **kw):
    from sr_gan_fd_amd import model as M
    from sr_gan_fd_amd.gan_esrgan import EsrganGanTrainer
    g, d = _pin(dt, M.RRDBNet(num_rrdb=1, upscale_factor=2), M.discriminator())
    cl = _pin(dt, M.ContentLoss("features.34", MEAN, STD))[0] if content else None
    tr = EsrganGanTrainer(g, d, cl, **kw)
    for _ in range(2):                 # the discriminator's ring of plans
        tr.step(torch.rand(2, 3, 64, 64), torch.rand(2, 3, 128, 128))
    return g, d, cl, tr


def _g_only(dt, num_rrdb=1, **kw):
    from sr_gan_fd_amd import model as M
    from sr_gan_fd_amd.trainer import GeneratorTrainer
    g, = _pin(dt, M.bsrgan_x4(num_rrdb=num_rrdb))
    tr = GeneratorTrainer(g, lr=1e-4, **kw)
    tr.step(torch.rand(2, 3, 16, 16), torch.rand(2, 3, 64, 64))
    return g, tr


def _modules(dt):
    """the module paths through autograd"""
    from sr_gan_fd_amd import model as M
    keep = []
    for dfac, shape in ((_unet, (2, 3, 32, 32)), (M.uNetDiscriminatorAesrgan, (2, 3, 32, 32)), (M.discriminator, (2, 3, 128, 128))):
        d, = _pin(dt, dfac())
        keep.append(d)
        x = torch.rand(*shape, requires_grad=True)
        d(x).sum().backward()                      # weights and dx
        for p in d.parameters():
            p.requires_grad_(False)
        d(x).sum().backward()                      # need_wgrad=False
        with torch.no_grad():
            d.eval()
            d(x)
    cl1, cl5 = _pin(dt, M.ContentLoss("features.34", MEAN, STD), M.ContentLoss(NODES, MEAN, STD))
    sr = torch.rand(2, 3, 32, 32, requires_grad=True)
    cl1(sr, torch.rand(2, 3, 32, 32)).backward()
    cl5(sr, torch.rand(2, 3, 32, 32))
    blk, = _pin(dt, M.BSRGAN(num_rrdb=1).trunk[0])
    xb = torch.rand(1, 64, 16, 16, requires_grad=True)
    blk(xb).sum().backward()
    return keep + [cl1, cl5, blk]


def _aesrgan():
    from sr_gan_fd_amd import model as M
    return M.uNetDiscriminatorAesrgan()


def _four_ways(m, x, result=lambda out: out):
    """a module's ``__call__`` under autograd in the four gradient configurations (tests/test_rpa_host.py::test_module_call_sequence)"""
    result(m(x)).sum().backward()                  # input and parameters
    for p in m.parameters():
        p.requires_grad_(False)
    result(m(x)).sum().backward()                  # parameters frozen: no weight-gradient launches
    with torch.no_grad():
        m(x.detach())                              # nothing wants a gradient: the forward alone
    for p in m.parameters():
        p.requires_grad_(True)
    result(m(x.detach())).sum().backward()         # parameters only: the input's gradient is not computed


def _rpa_blocks(dt):
    from sr_gan_fd_amd import model as M
    keep = _pin(dt, M.RPA(64), M.US(64, 2))
    for m in keep:
        _four_ways(m, torch.rand(2, 64, 5, 7, requires_grad=True))
    return keep


def _gen_rpa(dt):
    """odd, non-square sizes: swapped H and W in the engines' shell would show"""
    from sr_gan_fd_amd import model as M
    keep = _pin(dt, *(M.Generator_RPA(scale=s, num_block=2) for s in (1, 2, 4)))
    for m in keep:
        _four_ways(m, torch.rand(2, 3, 5, 7, requires_grad=True))
    return keep


def _self_attention(dt):
    from sr_gan_fd_amd import model as M
    m, = _pin(dt, M.SelfAttention(256, 8))
    for need_weights in (True, False):
        m.need_weights = need_weights
        _four_ways(m, torch.randn(2, 256, 4, 6, requires_grad=True), lambda out: out[0])
    return m,


SCENARIOS = {
    "gan_unet": lambda dt: _gan(dt, _unet),
    "gan_unet_generator_first": lambda dt: _gan(dt, _unet, True),
    "gan_aesrgan": lambda dt: _gan(dt, _aesrgan),
    "esrgan_gan": _esrgan,
    "generator_only": _g_only,
    "modules": _modules,
    # six dense blocks: one full batch of four slab reductions and a remainder of two, and the mid-trunk bucket marker (R >= 4)
    "generator_only_rrdb2": lambda dt: _g_only(dt, 2),
    # the pixel-attention generator's blocks alone and the generator at every scale (0, 1 and 2 US blocks), then SelfAttention with
    # and without the weights launch: each in the four gradient configurations of _four_ways
    "rpa_blocks": _rpa_blocks,
    "gen_rpa": _gen_rpa,
    "self_attention": _self_attention,
    # the trainers' remaining branches: a frozen generator, no content criterion, the generator-first order without a sharpened GT,
    # and no EMA copy
    "gan_unet_frozen_generator": lambda dt: _gan(dt, _unet, train_generator=False),
    "gan_unet_no_content": lambda dt: _gan(dt, _unet, content=False),
    "gan_unet_generator_first_no_usm": lambda dt: _gan(dt, _unet, True, usm=False),
    "esrgan_gan_no_content_no_ema": lambda dt: _esrgan(dt, content=False, ema_decay=None),
    "generator_only_no_ema": lambda dt: _g_only(dt, ema_decay=None),
}
CASES = ["%s-%s" % (s, d) for s in SCENARIOS for d in DTYPES]


class Brackets:
    """stands in for profiling.Recorder: notes the label and the algorithmic work of every bracketed launch, then makes it"""

    def __init__(self):
        self.items = []

    def bracket(self, label, work, fn):
        flops, nbytes = work if isinstance(work, tuple) else (work, 0.0)
        self.items.append([label, round(float(flops), 9), round(float(nbytes), 9)])
        fn()


def record(case, profiled=False):
    """run one scenario under the recorder: {"launches": [...], "queries": [...], "tables": [...]}; ``profiled``: with
    profiling.REC set -- the label queries are left out of the launches, and "brackets" holds [label, flop, bytes] per bracket"""
    from sr_gan_fd_amd import _abi as A, ops, profiling
    name, dt = case.rsplit("-", 1)
    A.set_dry_run(True)
    rec = Recorder(A.lib())
    ops._DC_WS.clear()                 # the process-wide dense-chain workspace: its size query belongs to the scenario that plans the first chain
    A._lib = rec
    assert profiling.REC is None
    if profiled:
        profiling.REC = Brackets()
    try:
        torch.manual_seed(0)
        keep = SCENARIOS[name](DTYPES[dt])
        out = {"launches": rec.launches, "queries": rec.queries, "tables": rec.tables()}
        if profiled:
            out["launches"] = [c for c in rec.launches if c[0] != "srganfd_conv2d_describe"]
            out["brackets"] = profiling.REC.items
        del keep
    finally:
        profiling.REC = None
        A._lib = rec._lib
        ops._DC_WS.clear()
        A.set_dry_run(False)
    return json.loads(json.dumps(out))          # tuples -> lists, as the fixture holds them


def _diff(want, got, path=""):
    """paths at which two JSON values differ, with both values"""
    if isinstance(want, dict) and isinstance(got, dict) and set(want) == set(got):
        return [d for k in want for d in _diff(want[k], got[k], "%s.%s" % (path, k))]
    if isinstance(want, list) and isinstance(got, list) and len(want) == len(got):
        return [d for i, (a, b) in enumerate(zip(want, got)) for d in _diff(a, b, "%s[%d]" % (path, i))]
    return [] if want == got else ["%s: recorded %s, now %s" % (path or "value", json.dumps(want)[:200], json.dumps(got)[:200])]


def compare(case, want, got):
    """None, or the description of the first difference"""
    for i, (a, b) in enumerate(zip(want["launches"], got["launches"])):
        if a != b:
            if a[0] != b[0]:
                return "%s: call %d was %s, is now %s" % (case, i, a[0], b[0])
            return "%s: call %d (%s) differs in\n  %s" % (case, i, a[0], "\n  ".join(_diff(a[1:], b[1:], "arg")))
    if len(want["launches"]) != len(got["launches"]):
        n = min(len(want["launches"]), len(got["launches"]))
        extra = (want if len(want["launches"]) > n else got)["launches"][n][0]
        return "%s: %d calls recorded, %d now; call %d (%s) is the first without a partner" % (case, len(want["launches"]), len(got["launches"]), n, extra)
    cw, cg = (Counter(json.dumps(q, sort_keys=True) for q in t["queries"]) for t in (want, got))
    if cw != cg:
        return "%s: plan-building queries differ: no longer made %s; new %s" % (case, sorted((cw - cg).elements())[:5], sorted((cg - cw).elements())[:5])
    d = _diff(want["tables"], got["tables"], "tables")
    if d:
        return "%s: pack tables differ in\n  %s" % (case, "\n  ".join(d[:10]))
    return None


@pytest.fixture(scope="module")
def recorded():
    with gzip.open(FIXTURE, "rt") as f:
        return json.load(f)


def test_fixture_covers_every_case(recorded):
    assert sorted(recorded) == sorted(CASES)
    assert sum(len(t["launches"]) + len(t["queries"]) for t in recorded.values()) > 8000
    assert os.path.getsize(FIXTURE) < 1 << 20


@pytest.mark.parametrize("case", CASES)
def test_launch_trace_matches_the_recorded_one(case, recorded):
    msg = compare(case, recorded[case], record(case))
    assert msg is None, msg


@pytest.fixture(scope="module")
def recorded_labels():
    with gzip.open(LABELS, "rt") as f:
        return json.load(f)


def test_label_fixture_covers_every_case(recorded_labels):
    assert sorted(recorded_labels) == sorted(CASES)
    assert sum(len(b) for b in recorded_labels.values()) > 3000
    assert os.path.getsize(LABELS) < 1 << 18


@pytest.mark.parametrize("case", CASES)
def test_profiled_path_launches_the_same_under_the_recorded_labels(case, recorded, recorded_labels):
    got = record(case, profiled=True)
    msg = compare(case, recorded[case], got)
    assert msg is None, "with profiling.REC set, " + msg
    want, have = recorded_labels[case], got["brackets"]
    for i, (a, b) in enumerate(zip(want, have)):
        assert a == b, "%s: bracket %d was %s, is now %s" % (case, i, a, b)
    assert len(want) == len(have), "%s: %d brackets recorded, %d now" % (case, len(want), len(have))
