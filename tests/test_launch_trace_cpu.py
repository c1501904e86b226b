"""Launch-trace snapshot of the HipGoNet planner, without a GPU.

Every native call of ``deep_go_amd/models/hip_model.py`` goes through ``self.h``.  With that
module replaced by a recording proxy (host-side shape queries pass through to the built
``_dghip``; every other call is recorded instead of run) and ``torch.cuda``'s streams and
events replaced by fakes, a ``HipGoNet`` builds on ``device="cpu"`` and "runs" whole steps:
the result is the exact launch sequence — function names, arguments, launch-table contents,
streams and cross-stream hand-offs — of construction (+ ``refresh_weights``), one eager
``SegmentedStep``, ``evaluate()`` and ``forward_backward(); optimizer_step()``.

Pointers are symbolised: an int that is the address of an int64 launch table becomes the
table's contents (recursively), an int inside a tensor storage reachable from ``vars(net)``
becomes ``buf<k>+<offset>`` (k = order of first appearance in the trace, so attribute names
and allocation order do not matter), a stream handle becomes its role (main / side / load).

The traces of all cases are compared with ``tests/fixtures/launch_traces.json``, which is a
recording, never edited by hand: a planner refactor must reproduce it byte for byte.
Regenerate (only for an intended change of the launch plan) with
``python tests/test_launch_trace_cpu.py --write``.

Coverage: the union of the traced names must include every ``h.<name>`` launch function
that hip_model.py mentions.  Nothing is out of reach on the CPU: ``UNREACHABLE`` is empty.
(Not traced because they are not launches of hip_model.py: the collectives of a real
bucketer — the fake one only records fire / wait / enqueue / join — and the hipGraph
capture, which replays what the eager step issues.)
"""
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from deep_go_amd.ops import native  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "fixtures", "launch_traces.json")
BATCH = 4        # the smallest batch with B % 4 == 0 (the fp8 window kernel's condition)
NUM_CUS = 256

# host-side queries answered by the real extension (everything else is a recorded launch)
PASS_PREFIXES = ("bias_chunks", "conv_wgrad_wgs_per_cu")
PASS_NAMES = {"conv_l1_ok", "conv_l1_frag_ok", "conv_wgrad_ktile", "conv_wgrad_win_splits",
              "conv_wgrad_win8_splits", "grad_update_cols", "grad_update_tickets"}
# launch functions named in hip_model.py that no CPU trace can reach (none)
UNREACHABLE = set()


def _is_query(name):
    return name in PASS_NAMES or name.startswith(PASS_PREFIXES) or name.startswith("EPI_")


class _RecordingHip:
    """Stands in for the ``_dghip`` module: one wrapper object per name (the planner compares
    launch functions with ``is`` / ``in``), each appending ``[name, *args]`` to the trace."""

    def __init__(self, real, trace):
        self._real, self._trace, self._fns = real, trace, {}

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        if _is_query(name):
            return getattr(self._real, name)
        getattr(self._real, name)       # a launch the extension does not have is an error
        fn = self._fns.get(name)
        if fn is None:
            def fn(*args, _name=name):
                self._trace.append([_name, *args])
            fn.__name__ = name
            self._fns[name] = fn
        return fn


class _Stream:
    """A fake torch.cuda.Stream: a handle and the recorded hand-offs."""
    _next = [0]

    def __init__(self, cuda, **_):
        self.cuda = cuda
        _Stream._next[0] += 1
        # far above any heap address; resolved to a role name when the trace is symbolised
        self.cuda_stream = (0x7A << 56) + _Stream._next[0]

    def wait_stream(self, other):
        self.cuda.trace.append(["wait_stream", self, other])

    def record_event(self):
        ev = _Event(self.cuda)
        self.cuda.trace.append(["record_event", self])
        ev.stream = self
        return ev

    def wait_event(self, ev):
        self.cuda.trace.append(["wait_event", self, ev.stream])


class _Event:
    def __init__(self, cuda=None, **_):
        self.cuda, self.stream = cuda, None

    def record(self, stream=None):
        self.stream = stream if stream is not None else self.cuda.cur
        self.cuda.trace.append(["Event.record", self.stream])


class _FakeCuda:
    """The torch.cuda entry points hip_model.py uses, over fake streams."""

    def __init__(self, trace):
        self.trace = trace
        self.main = _Stream(self)
        self.cur = self.main

    def Stream(self, **kw):
        return _Stream(self, **kw)

    def Event(self, **kw):
        return _Event(self, **kw)

    def current_stream(self, device=None):
        return self.cur

    def stream(self, s):
        cuda = self

        class _Ctx:
            def __enter__(self):
                self.prev, cuda.cur = cuda.cur, s

            def __exit__(self, *exc):
                cuda.cur = self.prev
        return _Ctx()

    def stream_handle(self, stream=None):
        return int((stream if stream is not None else self.cur).cuda_stream)


class _Bucketer:
    """A fake gradient bucketer: records when the step hands it a bucket."""

    def __init__(self, trace, buckets, in_graph):
        self.trace, self.buckets, self.in_graph = trace, buckets, in_graph

    def fire(self, b):
        self.trace.append(["bucket.fire", b])

    def wait(self):
        self.trace.append(["bucket.wait"])

    def enqueue(self, b):
        self.trace.append(["bucket.enqueue", b])

    def join(self):
        self.trace.append(["bucket.join"])


# ---------------------------------------------------------------- symbolising
def _walk(v, tensors, tables, seen):
    if id(v) in seen:
        return
    if isinstance(v, torch.Tensor):
        seen.add(id(v))
        st = v.untyped_storage()
        if st.nbytes():
            tensors[st.data_ptr()] = st.nbytes()
    elif isinstance(v, np.ndarray):
        seen.add(id(v))
        if v.dtype == np.int64 and v.size:
            tables[v.ctypes.data] = v
    elif isinstance(v, (list, tuple, set)):
        seen.add(id(v))
        for x in v:
            _walk(x, tensors, tables, seen)
    elif isinstance(v, dict):
        seen.add(id(v))
        for x in v.values():
            _walk(x, tensors, tables, seen)


class _Symboliser:
    def __init__(self, net, cuda):
        self.tensors, self.tables = {}, {}
        _walk(vars(net), self.tensors, self.tables, set())
        self.bases = sorted(self.tensors)
        self.names = {}
        self.roles = {id(cuda.main): "main"}
        if getattr(net, "side", None) is not None:
            self.roles[id(net.side)] = "side"
        if getattr(net, "load_stream", None) is not None:
            self.roles[id(net.load_stream)] = "load"
        self.handles = {s.cuda_stream: r for s, r in (
            (cuda.main, "main"), (getattr(net, "side", None), "side"),
            (getattr(net, "load_stream", None), "load")) if s is not None}

    def __call__(self, v, depth=0):
        if isinstance(v, _Stream):
            return self.roles[id(v)]
        if isinstance(v, (bool, np.bool_)):
            return int(v)
        if isinstance(v, (int, np.integer)):
            v = int(v)
            if v in self.handles:
                return self.handles[v]
            if v in self.tables and depth < 4:
                t = self.tables[v]
                return {"table": [[self(x, depth + 1) for x in row]
                                  for row in t.reshape(len(t), -1).tolist()]}
            k = int(np.searchsorted(self.bases, v, side="right")) - 1
            if k >= 0 and v < self.bases[k] + self.tensors[self.bases[k]]:
                base = self.bases[k]
                if base not in self.names:
                    self.names[base] = f"buf{len(self.names)}"
                return f"{self.names[base]}+{v - base}"
            return v
        if isinstance(v, (float, np.floating)):
            return float(v)
        if isinstance(v, (list, tuple)):
            return [self(x, depth) for x in v]
        if isinstance(v, str) or v is None:
            return v
        raise TypeError(f"unexpected launch argument {v!r}")


# ---------------------------------------------------------------- cases
def _case(layers, ch, dtype="bf16", env=None, cfg=None, net=None, mode="single"):
    return dict(layers=layers, ch=ch, dtype=dtype, env=env or {}, cfg=cfg or {},
                net=net or {}, mode=mode)


_DP = dict(net=dict(grad_wire="bf16", global_batch=2 * BATCH, wgrad_group=2))


def _cases():
    c = {}
    for ch in (128, 256):
        for dt in ("bf16", "fp8"):
            c[f"5x{ch}-{dt}"] = _case(5, ch, dt)
    c["4x64-bf16"] = _case(4, 64)
    c["12x128-bf16"] = _case(12, 128)
    c["5x128-bf16-dp"] = _case(5, 128, mode="dp", **_DP)
    c["5x256-fp8-dp-ingraph"] = _case(5, 256, "fp8", mode="dp-ingraph", **_DP)
    c["5x128-bf16-dp-fp32"] = _case(5, 128, mode="dp",
                                    net=dict(global_batch=2 * BATCH, wgrad_group=2))
    c["5x128-bf16-prefetch"] = _case(5, 128, mode="prefetch")
    c["5x256-fp8-prefetch"] = _case(5, 256, "fp8", mode="prefetch")
    # layers the board kernels refuse: pixel-tiled forward (conv_nt_ex) and dgrad (conv_nt)
    c["4x64-k5-hidden"] = _case(4, 64, cfg=dict(hidden_kernel=5))
    c["4x96-bf16"] = _case(4, 96)
    c["5x128-bf16-rmsprop"] = _case(5, 128, cfg=dict(optimizer="rmsprop", rate=1e-3))
    c["5x128-bf16-raise"] = _case(5, 128, cfg=dict(nan_policy="raise"))
    c["5x128-bf16-no-head-relu"] = _case(5, 128, cfg=dict(head_relu=False))
    c["5x128-fp8-keep-frames"] = _case(5, 128, "fp8", net=dict(keep_act_frames=True))
    c["5x128-bf16-group2"] = _case(5, 128, net=dict(wgrad_group=2))
    knobs = [
        ("DG_STACK", "0", [(5, 128, "bf16"), (5, 128, "fp8"), (5, 256, "fp8")]),
        ("DG_DSTACK", "0", [(5, 128, "bf16"), (5, 128, "fp8")]),
        ("DG_STACK_L1", "0", [(5, 128, "bf16")]),
        ("DG_L1_FRAG", "0", [(5, 256, "bf16"), (5, 128, "fp8")]),
        ("DG_LAYER2", "0", [(5, 256, "bf16")]),
        ("DG_LAYER2_MULTI", "0", [(5, 256, "bf16")]),
        ("DG_FUSE_HEAD", "0", [(5, 128, "bf16"), (5, 256, "bf16"), (5, 256, "fp8")]),
        ("DG_RELU_MASK", "0", [(5, 128, "bf16"), (5, 256, "bf16")]),
        ("DG_L0_MASK", "0", [(5, 128, "bf16")]),
        ("DG_L0_MASK", "1", [(5, 128, "bf16")]),
        ("DG_L0_BIAS_SMALL", "0", [(5, 128, "bf16"), (5, 256, "bf16")]),
        ("DG_DGRAD_FIRST", "0", [(5, 128, "bf16"), (5, 256, "bf16")]),
        ("DG_WGRAD_GROUP", "1", [(5, 128, "bf16")]),
        ("DG_WGRAD_GROUP", "2", [(5, 128, "bf16"), (5, 256, "fp8")]),
        ("DG_WGRAD_WIN", "0", [(5, 128, "bf16"), (5, 256, "fp8")]),
        ("DG_SIDE_STREAM", "0", [(5, 128, "bf16"), (5, 256, "bf16")]),
        ("DG_SIDE_STREAM", "bias", [(5, 128, "bf16")]),
        ("DG_FUSED_UPDATE", "0", [(5, 128, "bf16"), (5, 256, "fp8")]),
        ("DG_EARLY_UPDATE", "0", [(5, 256, "bf16"), (5, 256, "fp8")]),
        ("DG_EARLY_UPDATE", "1", [(5, 128, "bf16")]),
        ("DG_FP8_DGRAD", "0", [(5, 128, "fp8"), (5, 256, "fp8")]),
        ("DG_FP8_WGRAD", "0", [(5, 128, "fp8"), (5, 256, "fp8")]),
        ("DG_FP8_SR", "0", [(5, 128, "fp8")]),
    ]
    for name, val, shapes in knobs:
        for layers, ch, dt in shapes:
            c[f"{layers}x{ch}-{dt}-{name[3:]}={val}"] = _case(layers, ch, dt, env={name: val})
    # a 7x7 first layer runs pixel-tiled (conv_nt_ex): DG_L0_MASK=1 opts its ReLU bits in
    c["5x128-bf16-k7-first"] = _case(5, 128, cfg=dict(first_kernel=7))
    c["5x128-bf16-k7-first-L0_MASK=1"] = _case(5, 128, cfg=dict(first_kernel=7),
                                               env={"DG_L0_MASK": "1"})
    # the board kernel's M tile shows where the per-layer board kernel runs
    c["5x128-bf16-STACK=0-BOARD_BM=128"] = _case(5, 128, env={
        "DG_STACK": "0", "DG_DSTACK": "0", "DG_BOARD_BM": "128"})
    c["5x256-bf16-LAYER2=0-BOARD_BM=128"] = _case(5, 256, env={
        "DG_LAYER2": "0", "DG_BOARD_BM": "128"})
    # several knobs at once: every per-layer kernel (no stack, run or group)
    c["5x128-bf16-per-layer"] = _case(5, 128, env={
        "DG_STACK": "0", "DG_DSTACK": "0", "DG_DGRAD_FIRST": "0", "DG_WGRAD_GROUP": "1"})
    c["5x256-bf16-per-layer"] = _case(5, 256, env={
        "DG_LAYER2": "0", "DG_DGRAD_FIRST": "0", "DG_WGRAD_GROUP": "1", "DG_L1_FRAG": "0"})
    # the separate optimizer launches: rmsprop, and both on the bf16 wire
    c["5x128-bf16-rmsprop-FUSED_UPDATE=0"] = _case(
        5, 128, env={"DG_FUSED_UPDATE": "0"}, cfg=dict(optimizer="rmsprop", rate=1e-3))
    c["5x128-bf16-dp-FUSED_UPDATE=0"] = _case(5, 128, mode="dp",
                                              env={"DG_FUSED_UPDATE": "0"}, **_DP)
    c["5x128-bf16-dp-rmsprop-FUSED_UPDATE=0"] = _case(
        5, 128, mode="dp", env={"DG_FUSED_UPDATE": "0"},
        cfg=dict(optimizer="rmsprop", rate=1e-3), **_DP)
    return c


CASES = _cases()


def _trace_case(case, monkeypatch):
    """The symbolised trace of one case: {phase: [[name, *args], ...]}."""
    from deep_go_amd.config import get_preset
    from deep_go_amd.data.batch import packed_batch_bytes
    from deep_go_amd.models import hip_model
    for k in list(os.environ):
        if k.startswith("DG_"):
            monkeypatch.delenv(k)
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    trace = []
    cuda = _FakeCuda(trace)
    rec = _RecordingHip(native.hip(), trace)
    monkeypatch.setattr(hip_model, "hip", lambda: rec)
    monkeypatch.setattr(hip_model, "stream_handle", cuda.stream_handle)
    for name in ("Stream", "Event", "current_stream", "stream"):
        monkeypatch.setattr(torch.cuda, name, getattr(cuda, name))
    cfg = get_preset("12x128-bf16", numLayers=case["layers"], channelSize=case["ch"],
                     batchSize=BATCH, dtype=case["dtype"], **case["cfg"])
    marks = {}
    net = hip_model.HipGoNet(cfg, BATCH, device="cpu", num_cus=NUM_CUS, **case["net"])
    net._fp8_calibrated = True
    marks["construct"] = len(trace)
    mode = case["mode"]
    bucketer = None
    if mode.startswith("dp"):
        # buckets (start, end, lowest layer): head + top group | the middle layers | layer 0
        L = net.L
        buckets = [(0, 0, L - 1), (0, 0, L - 3), (0, 0, 1), (0, 0, 0)]
        bucketer = _Bucketer(trace, buckets, in_graph=mode == "dp-ingraph")
    if mode == "prefetch":
        net.enable_prefetch()
    step = hip_model.SegmentedStep(net, bucketer, use_graphs=False)
    if mode == "prefetch":
        for k in range(2):       # both input buffers
            net.set_batch_packed(torch.zeros(packed_batch_bytes(BATCH), dtype=torch.uint8))
            step()
            marks[f"load+step{k}"] = len(trace)
    else:
        step()
        marks["step"] = len(trace)
    if bucketer is None:
        net.evaluate()
        marks["evaluate"] = len(trace)
        net.forward_backward()
        net.optimizer_step()
        marks["forward_backward+optimizer_step"] = len(trace)
    sym = _Symboliser(net, cuda)
    out, start = {}, 0
    for phase, end in marks.items():
        out[phase] = [sym(call) for call in trace[start:end]]
        start = end
    return out


def _dump(traces):
    """The fixture's text: every distinct call once (most cases share most launches), and
    per case and phase the indices of its calls in order."""
    calls, index, cases = [], {}, {}
    for name in sorted(traces):
        cases[name] = {}
        for phase, seq in traces[name].items():
            keys = [json.dumps(call, separators=(",", ":")) for call in seq]
            for k, call in zip(keys, seq):
                if k not in index:
                    index[k] = len(calls)
                    calls.append(call)
            cases[name][phase] = [index[k] for k in keys]
    return json.dumps({"calls": calls, "cases": cases}, separators=(",", ":")) + "\n"


def _load(text):
    d = json.loads(text)
    return {name: {phase: [d["calls"][k] for k in seq] for phase, seq in phases.items()}
            for name, phases in d["cases"].items()}


def _launch_names_in_planner():
    from deep_go_amd.models import hip_model
    src = inspect.getsource(hip_model)
    return {n for n in re.findall(r"\bh\.([A-Za-z_]\w*)", src) if not _is_query(n)}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return _load(f.read())


def _need_ext():
    if not native.hip_available():
        pytest.skip("_dghip is not built")


def test_cases_match_fixture(recorded):
    assert sorted(recorded) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_trace(name, recorded, monkeypatch):
    _need_ext()
    got = _load(_dump({name: _trace_case(CASES[name], monkeypatch)}))[name]
    want = recorded[name]
    assert list(got) == list(want)
    for phase in want:
        for k, (g, w) in enumerate(zip(got[phase], want[phase])):
            assert g == w, f"{name} / {phase} / call {k}"
        assert len(got[phase]) == len(want[phase]), f"{name} / {phase}"


def test_every_launch_function_is_traced(recorded):
    _need_ext()
    traced = {call[0] for case in recorded.values() for calls in case.values()
              for call in calls}
    want = _launch_names_in_planner() - UNREACHABLE
    assert len(want) > 40          # (the scan found the planner's launches)
    assert not (want - traced), sorted(want - traced)


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_launch_trace_cpu.py --write")
    traces = {}
    for name, case in sorted(CASES.items()):
        mp = pytest.MonkeyPatch()
        try:
            traces[name] = _trace_case(case, mp)
        finally:
            mp.undo()
    text = _dump(traces)
    with open(FIXTURE, "w") as f:
        f.write(text)
    print(f"{len(traces)} cases, {len(text)} bytes -> {FIXTURE}")
