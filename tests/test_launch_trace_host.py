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

Which buffer: a wrong activation or gradient buffer wired into a launch, or two buffers that alias, leaves every ``"p"`` of the trace
a ``"p"``.  A third fixture, tests/golden/launch_buffers.json.gz (``python tests/golden/make_golden_launch_buffers.py``, same rule),
holds per launch one entry for every pointer the trace records as ``"p"``, in the order the trace canonicalises them:
``"a<k>+<byte offset>"`` when the pointer falls inside the storage of a tensor that a cached plan (``eng.shapes``) of an engine alive
at the time of the call keeps alive, else ``"p"`` (per-call inputs and outputs, flat gradients, what the trainers own).  The plans
are walked through dicts, lists, tuples, sets and objects with ``__dict__`` or ``__slots__``, stopping at modules, ctypes objects and
engines; the recorder keeps every storage it has found until the scenario ends, so no later buffer gets a named one's address, and
``k`` counts the storages in the order in which the scenario's launches first point into them.  The calls that only ask the library
something (QUERIES) are compared without an order and are not part of this fixture.
"""
import bisect
import ctypes as C
import gzip
import hashlib
import json
import os
import weakref
from collections import Counter

import pytest
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_trace.json.gz")
BUFFERS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_buffers.json.gz")
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


def _plan_storages(found):
    """adds to ``found`` (address -> storage) the storage of every tensor that a cached plan of an engine alive now holds"""
    from sr_gan_fd_amd import engine as E
    seen = set()
    todo = [sp for eng in list(E._ENGINES.values()) for sp, _ in list(eng.shapes.d.values())]
    while todo:
        o = todo.pop()
        if id(o) in seen or type(o) in weakref.ProxyTypes or o is None or isinstance(o, (str, bytes, int, float, torch.dtype, torch.device)):
            continue
        seen.add(id(o))
        if isinstance(o, torch.Tensor):
            st = o.untyped_storage()
            if st.nbytes():
                found.setdefault(st.data_ptr(), st)
        elif isinstance(o, dict):
            todo.extend(o.values())
        elif isinstance(o, (list, tuple, set, frozenset)):
            todo.extend(o)
        elif not isinstance(o, (torch.nn.Module, E.EngineBase, C.Structure, C.Union, C.Array, C._SimpleCData, C._Pointer, type)):
            todo.extend(getattr(o, "__dict__", {}).values())
            todo.extend(getattr(o, n) for c in type(o).__mro__ for n in getattr(c, "__slots__", ()) if hasattr(o, n))


class Recorder:
    """stands in for the CDLL object: records every srganfd_* call, then makes it"""

    def __init__(self, lib, buffers=False):
        self._lib, self._wrapped = lib, {}
        self.launches, self.queries = [], []
        self._bufs = None
        # the plan-held buffers (module docstring): storages found so far by address, their sorted addresses, the names given, and per
        # launch the entries of its "p" pointers
        self.buffers = [] if buffers else None
        self._held, self._bases, self._names, self._row = {}, [], {}, None

    def _plan_buffer(self, v):
        for walked in (False, True):
            i = bisect.bisect_right(self._bases, v) - 1
            if i >= 0 and v < self._bases[i] + self._held[self._bases[i]].nbytes():
                base = self._bases[i]
                return "a%d+%d" % (self._names.setdefault(base, len(self._names)), v - base)
            if not walked:                                     # not in a storage found so far: look at the plans as they are now
                _plan_storages(self._held)
                self._bases = sorted(self._held)
        return "p"

    def _ptr(self, v):
        if not v:
            return None
        if self._bufs is None:
            self._bufs = _engine_buffers()
        for base, nbytes, name in self._bufs:
            if base <= v < base + nbytes:
                return "%s+%d" % (name, v - base)
        if self._row is not None:
            self._row.append(self._plan_buffer(v))
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
                if self.buffers is not None and dest is self.launches:
                    self._row = []
                    self.buffers.append(self._row)
                dest.append([name] + [self._canon(a, types[i] if i < len(types) else None) for i, a in enumerate(args)])
                self._row = None
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


def _bsrgantrans(dt):
    """the stage between trunk and conv2 (engine_trans.py over transformer.py's layers), dropout sites drawing: in dry-run mode no
    mask is drawn, so the record does not depend on the random stream"""
    import contextlib
    import io
    from sr_gan_fd_amd import model as M
    with contextlib.redirect_stdout(io.StringIO()):
        m, = _pin(dt, M.bsrgantrans_x2(num_rrdb=1).train())
    _four_ways(m, torch.rand(2, 3, 8, 8, requires_grad=True))
    return m,


def _transformer_encoder(dt):
    """the shape of tests/test_transformer_host.py::test_module_call_sequence_at_the_consumers_shape, training mode (dropout launches)"""
    from sr_gan_fd_amd import model as M
    m, = _pin(dt, M.TransformerEncoder(M.TransformerEncoderLayer(64, 4, 2048, 0.1), 2).train())
    _four_ways(m, torch.randn(8, 900, 64, requires_grad=True))
    return m,


def _realesrgan_x2(dt):
    """PixelUnshuffle(2) in front of conv1 (12 channels, padded to 32), through the module path: a training step, then a forward alone"""
    from sr_gan_fd_amd import model as M
    g, = _pin(dt, M.RRDBNet(num_rrdb=1, upscale_factor=2))
    g(torch.rand(2, 3, 12, 20)).sum().backward()
    with torch.no_grad():
        g(torch.rand(2, 3, 12, 20))
    return g,


def _trunk_inference(dt):
    """six dense blocks on an inference plan: block 0's buffer and the four that rotate"""
    from sr_gan_fd_amd import model as M
    g, = _pin(dt, M.bsrgan_x4(num_rrdb=2))
    with torch.no_grad():
        g(torch.rand(2, 3, 10, 6))
    return g,


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
    # the planners the cases above do not reach: the transformer stage inside the generator and the encoder stack alone, a generator
    # with PixelUnshuffle in front, and the generator's inference plan with its rotating dense-block buffers
    "bsrgantrans_x2": _bsrgantrans,
    "transformer_encoder": _transformer_encoder,
    "realesrgan_x2_module": _realesrgan_x2,
    "generator_inference_rrdb2": _trunk_inference,
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


def record(case, profiled=False, buffers=False):
    """run one scenario under the recorder: {"launches": [...], "queries": [...], "tables": [...]}; ``profiled``: with
    profiling.REC set -- the label queries are left out of the launches, and "brackets" holds [label, flop, bytes] per bracket;
    ``buffers``: "buffers" holds, per launch, the entries of the plan-held buffers (module docstring)"""
    from sr_gan_fd_amd import _abi as A, ops, profiling
    name, dt = case.rsplit("-", 1)
    A.set_dry_run(True)
    rec = Recorder(A.lib(), buffers)
    ops._DC_WS.clear()                 # the process-wide dense-chain workspace: its size query belongs to the scenario that plans the first chain
    A._lib = rec
    assert profiling.REC is None
    if profiled:
        profiling.REC = Brackets()
    try:
        torch.manual_seed(0)
        keep = SCENARIOS[name](DTYPES[dt])
        out = {"launches": rec.launches, "queries": rec.queries, "tables": rec.tables()}
        if buffers:
            out["buffers"] = rec.buffers
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


def compare_buffers(case, want, got):
    """None, or the description of the first launch whose plan-held buffers differ"""
    for i, (a, b) in enumerate(zip(want, got["buffers"])):
        if a != b:
            return "%s: call %d (%s) takes other plan buffers: recorded %s, now %s" % (case, i, got["launches"][i][0], json.dumps(a), json.dumps(b))
    if len(want) != len(got["buffers"]):
        return "%s: buffers of %d calls recorded, %d calls now" % (case, len(want), len(got["buffers"]))
    return None


@pytest.fixture(scope="module")
def recorded():
    with gzip.open(FIXTURE, "rt") as f:
        return json.load(f)


@pytest.fixture(scope="module")
def now():
    """case -> its record with the plan-held buffers: each case runs once for the trace test and the buffer test"""
    done = {}
    return lambda case: done[case] if case in done else done.setdefault(case, record(case, buffers=True))


def test_fixture_covers_every_case(recorded):
    assert sorted(recorded) == sorted(CASES)
    assert sum(len(t["launches"]) + len(t["queries"]) for t in recorded.values()) > 8000
    assert os.path.getsize(FIXTURE) < 1 << 20


@pytest.mark.parametrize("case", CASES)
def test_launch_trace_matches_the_recorded_one(case, recorded, now):
    msg = compare(case, recorded[case], now(case))
    assert msg is None, msg


@pytest.fixture(scope="module")
def recorded_buffers():
    with gzip.open(BUFFERS, "rt") as f:
        return json.load(f)


def test_buffer_fixture_covers_every_case(recorded, recorded_buffers):
    assert sorted(recorded_buffers) == sorted(CASES)
    assert all(len(recorded_buffers[c]) == len(recorded[c]["launches"]) for c in CASES)
    names = [e for rows in recorded_buffers.values() for row in rows for e in row]
    assert len(names) > 20000 and sum(e != "p" for e in names) > 0.8 * len(names)
    assert os.path.getsize(BUFFERS) < 1 << 16


@pytest.mark.parametrize("case", CASES)
def test_launches_take_the_recorded_plan_buffers(case, recorded_buffers, now):
    msg = compare_buffers(case, recorded_buffers[case], now(case))
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
