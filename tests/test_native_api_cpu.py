"""The Python-visible interface of the ``_dghip`` extension, pinned without a GPU.

``csrc/kernels/bindings.cpp`` derives most bindings from the C declarations in
``csrc/kernels/dg_api.h``; the launch-trace test records what the planner passes but never
calls the real functions.  These tests close the gap between the two on the CPU:

* ``tests/fixtures/native_signatures.json`` maps every public name of ``_dghip`` to the first
  line of its pybind ``__doc__`` (the generated signature) or, for an integer attribute, to
  its value.  The built module must match it exactly: a binding that gains, loses or retypes
  an argument, or a name that appears or disappears, fails here.  Like the trace fixture it
  is a recording, never edited by hand.  It was recorded from the hand-written bindings, at
  the commit before they were derived from ``dg_api.h``, with
  ``python tests/test_native_api_cpu.py --write device_sync last_error``
  (names after ``--write`` are left out: that change removed these two, which nothing
  called).  Regenerate only for an intended change of the interface.
* ``tests/fixtures/native_signatures_small.json`` does the same for the seven small modules
  (``_dgaug``, ``_dgopt``, ``_dgadam``, ``_dglamb``, ``_dgclip``, ``_dgema``, ``_dgsched``), with
  the full ``__doc__`` of every public name and of the module itself (key ``__doc__``).  It was
  recorded from their hand-written bindings, at the commit before they moved to the shared
  adapter of ``csrc/kernels/dg_bind.h``, with
  ``python tests/test_native_api_cpu.py --write-small``.
* every call recorded in ``tests/fixtures/launch_traces.json`` fits the signature of the
  function it names: the argument count, no ``float`` at an integer position, and pointers
  (symbolised buffers, tables, streams) only at integer positions.
* the adapter's error path (``RuntimeError("<name>: <hipGetErrorString>")``), its argument
  conversion (``TypeError`` for a float where an int is declared) and its value-returning
  branch, through launchers that validate and return before any GPU work.
"""
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from deep_go_amd.ops import native  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "fixtures", "native_signatures.json")
FIXTURE_SMALL = os.path.join(ROOT, "tests", "fixtures", "native_signatures_small.json")
SMALL = ("aug", "opt", "adam", "lamb", "clip", "ema", "sched")      # native.<name>() -> _dg<name>
TRACES = os.path.join(ROOT, "tests", "fixtures", "launch_traces.json")

# trace entries that are not native calls (the fakes of tests/test_launch_trace_cpu.py)
NOT_NATIVE = {"wait_stream", "wait_event", "record_event", "Event.record"}
NOT_NATIVE_PREFIX = "bucket."


def _interface(mod):
    """{public name: first line of the pybind doc (functions) | value (int attributes)}."""
    out = {}
    for name in dir(mod):
        if name.startswith("_"):
            continue
        v = getattr(mod, name)
        out[name] = v if isinstance(v, int) else v.__doc__.splitlines()[0]
    return out


def _interface_full(mod):
    """{public name: full pybind doc | value (int attributes)} + the module's own __doc__."""
    out = {"__doc__": mod.__doc__}
    for name in dir(mod):
        if not name.startswith("_"):
            v = getattr(mod, name)
            out[name] = v if isinstance(v, int) else v.__doc__
    return out


def _params(signature):
    """'f(arg0: int, arg1: float) -> None' -> ['int', 'float'] (pybind11 3 spells the two
    kinds 'typing.SupportsInt | typing.SupportsIndex' and 'typing.SupportsFloat | ...')."""
    inner = re.fullmatch(r"\w+\((.*)\) -> \w+", signature).group(1)
    kinds = []
    for p in inner.split(", ") if inner else []:
        annotation = p.split(": ")[1]
        is_int = annotation == "int" or annotation.startswith("typing.SupportsInt")
        is_float = annotation == "float" or annotation.startswith("typing.SupportsFloat")
        assert is_int or is_float, signature
        kinds.append("int" if is_int else "float")
    return kinds


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture
def h():
    if not native.hip_available():
        pytest.skip("_dghip is not built")
    return native.hip()


def test_module_matches_recorded_interface(h, recorded):
    got = _interface(h)
    assert sorted(got) == sorted(recorded)
    for name, want in recorded.items():
        assert got[name] == want, name


@pytest.mark.parametrize("name", SMALL)
def test_small_module_matches_recorded_interface(name):
    try:
        mod = getattr(native, name)()
    except native.NativeExtensionMissing:
        pytest.skip(f"_dg{name} is not built")
    with open(FIXTURE_SMALL) as f:
        want = json.load(f)["_dg" + name]
    got = _interface_full(mod)
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert got[k] == v, k


def test_recorded_launches_fit_the_signatures(recorded):
    with open(TRACES) as f:
        calls = json.load(f)["calls"]
    checked = set()
    for call in calls:
        name, args = call[0], call[1:]
        if name in NOT_NATIVE or name.startswith(NOT_NATIVE_PREFIX):
            continue
        assert isinstance(recorded.get(name), str), f"{name} is not a function of _dghip"
        kinds = _params(recorded[name])
        assert len(args) == len(kinds), f"{name}: {len(args)} arguments for {recorded[name]}"
        for k, (a, kind) in enumerate(zip(args, kinds)):
            if kind == "int":
                assert not isinstance(a, float), f"{name}: float {a} at integer argument {k}"
            else:
                assert isinstance(a, (int, float)), f"{name}: {a!r} at float argument {k}"
        checked.add(name)
    assert len(checked) >= 40          # (the fixture's launches were found)


CONV_WGRAD_KP1 = (3, 0, 1, 128, 128, 0, 1, 128, 4, 1, 1, 0, 0)      # KP = 1 (argument 9)
GRAD_UPDATE_ZERO = (0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0, 0, 0.0, 0, 0, 0, 0, 0, 0, 0)


@pytest.mark.parametrize("name, args", [
    ("weight_refresh", (0, 0, 0)),
    ("wgrad_reduce_multi", (0, 0, 0)),
    ("conv_wgrad", CONV_WGRAD_KP1),
    ("grad_update", GRAD_UPDATE_ZERO),
])
def test_invalid_launch_raises_with_the_binding_name(h, name, args):
    with pytest.raises(RuntimeError) as e:
        getattr(h, name)(*args)
    assert str(e.value) == f"{name}: invalid argument"


def test_float_for_an_int_is_a_type_error(h):
    args = list(CONV_WGRAD_KP1)
    args[9] = 1.5
    with pytest.raises(TypeError):
        h.conv_wgrad(*args)


def test_queries_return_values(h):
    assert h.bias_chunks(4) == 1
    assert h.grad_update_cols() == 29


if __name__ == "__main__":
    if sys.argv[1:] == ["--write-small"]:
        small = {"_dg" + n: _interface_full(getattr(native, n)()) for n in SMALL}
        with open(FIXTURE_SMALL, "w") as f:
            json.dump(small, f, indent=0, sort_keys=True)
            f.write("\n")
        sys.exit(print(f"{len(small)} modules -> {FIXTURE_SMALL}"))
    if sys.argv[1:2] != ["--write"]:
        sys.exit("usage: python tests/test_native_api_cpu.py --write [NAME_TO_LEAVE_OUT ...]\n"
                 "       python tests/test_native_api_cpu.py --write-small")
    iface = {k: v for k, v in _interface(native.hip()).items() if k not in sys.argv[2:]}
    with open(FIXTURE, "w") as f:
        json.dump(iface, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(iface)} names -> {FIXTURE}")
