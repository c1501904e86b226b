"""In-tree native build: hipcc for the gfx950 kernels, g++ for the CPU engine.

Produces, under ``deep_go_amd/_native/`` (in-tree, so the ``.so`` files travel with the tree):

* ``_dghip<EXT>``: the HIP kernels of the network (``HIP_SOURCES``), pybind11;
* ``_dg<name><EXT>`` for every row of ``SMALL``: one kernel file and its bindings each, apart
  from ``_dghip`` and from one another because the interface of each is recorded or pinned by
  tests, and imported only when the feature is asked for;
* ``_dgcpu<EXT>``: Go engine, t7 codec, SGF parser, loader thread pool;
* ``_dgcomm<EXT>``: the native RCCL communicator.

Usage: ``python -m deep_go_amd._build [--force] [--only hip|<a name of SMALL>|cpu|comm]
[--sanitize thread|address]``
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import os
import subprocess
import sys
import sysconfig
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "deep_go_amd"
OUT = PKG / "_native"
BUILD = ROOT / "build"
KDIR = ROOT / "csrc" / "kernels"
EDIR = ROOT / "csrc" / "engine"
CDIR = ROOT / "csrc" / "comm"
ARCH = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CXX = os.environ.get("CXX", "g++")
EXT = sysconfig.get_config_var("EXT_SUFFIX") or ".so"

HIP_SOURCES = ["conv_mfma.hip", "conv_board.hip", "conv_stack2.hip", "conv_layer2.hip", "conv_stack_f8.hip", "conv_wgrad_win.hip", "conv_wgrad_win8.hip", "conv_l1.hip", "conv_fp8.hip", "head.hip", "head_mfma.hip", "elementwise.hip", "policy.hip", "bindings.cpp"]
# the kernels' compile flags (tools/kloop_report.py compiles with the same ones)
HIP_FLAGS = [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics",
             "-Wno-unused-result"]
# the small modules _dg<name>: name -> (kernel file, bindings file).  ops/native.py's accessors
# and __graft_entry__.build() go by this table too.
SMALL = {
    "aug": ("augment.hip", "aug_bindings.cpp"),     # on-device D4 batch augmentation
    "opt": ("optim.hip", "opt_bindings.cpp"),       # SGD with momentum / Nesterov / weight decay
    "adam": ("optim.hip", "adam_bindings.cpp"),     # AdamW
    "lamb": ("optim.hip", "lamb_bindings.cpp"),     # LAMB
    "clip": ("clip.hip", "clip_bindings.cpp"),      # gradient clipping by the global norm
    "ema": ("ema.hip", "ema_bindings.cpp"),         # the moving average of the weights
    "sched": ("sched.hip", "sched_bindings.cpp"),   # the learning-rate schedule's launch
    "play": ("play.hip", "play_bindings.cpp"),      # move selection: temperature, top-p, draw
}
CPU_SOURCES = ["go_engine.cpp", "sgf.cpp", "t7.cpp", "features.cpp", "loader.cpp",
               "bindings.cpp"]


def _pybind_includes():
    import pybind11
    return [f"-I{pybind11.get_include()}", f"-I{sysconfig.get_paths()['include']}"]


def _newer(src: Path, dst: Path, deps=()) -> bool:
    if not dst.exists():
        return True
    t = dst.stat().st_mtime
    return src.stat().st_mtime > t or any(d.stat().st_mtime > t for d in deps)


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"build failed: {' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
    return r


def _objects(prefix: str, sources, force: bool, jobs: int) -> list[Path]:
    """build/<prefix>_<source>.o of each of KDIR's sources (.hip: device code with HIP_FLAGS,
    .cpp: pybind11 host code), the stale ones compiled in a thread pool."""
    BUILD.mkdir(exist_ok=True)
    headers = list(KDIR.glob("*.h"))
    objs, cmds = [], []
    for s in sources:
        src, obj = KDIR / s, BUILD / f"{prefix}_{s}.o"
        objs.append(obj)
        if force or _newer(src, obj, headers):
            flags = HIP_FLAGS if s.endswith(".hip") else ["-O2", "-std=c++17", "-fPIC",
                                                          *_pybind_includes()]
            cmds.append([HIPCC, *flags, "-c", str(src), "-o", str(obj)])
    with cf.ThreadPoolExecutor(max_workers=jobs) as ex:
        list(ex.map(_run, cmds))
    return objs


def _link(name: str, objs, force: bool) -> Path:
    """_native/_dg<name><EXT> from the objects, when one of them is newer than it."""
    OUT.mkdir(exist_ok=True)
    target = OUT / f"_dg{name}{EXT}"
    if force or any(_newer(o, target) for o in objs):
        _run([HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "--hip-link", "-o",
              str(target), *map(str, objs)])
    return target


def build_hip(force: bool = False, jobs: int = 8) -> Path:
    return _link("hip", _objects("hip", HIP_SOURCES, force, jobs), force)


def build_smalls(names, force: bool = False, jobs: int = 8) -> list[Path]:
    """The small modules named: every distinct source is compiled once (optim.hip is in three
    modules) and its object linked into each module that lists it."""
    sources = sorted({s for n in names for s in SMALL[n]})
    obj = dict(zip(sources, _objects("small", sources, force, jobs)))
    return [_link(n, [obj[s] for s in SMALL[n]], force) for n in names]


def build_small(name: str, force: bool = False) -> Path:
    return build_smalls([name], force)[0]


def build_cpu(force: bool = False, jobs: int = 8, sanitize: str | None = None) -> Path:
    BUILD.mkdir(exist_ok=True)
    OUT.mkdir(exist_ok=True)
    suffix = f"_{sanitize}" if sanitize else ""
    target = OUT / f"_dgcpu{suffix}{EXT}"
    headers = list(EDIR.glob("*.h"))
    flags = ["-O3", "-std=c++17", "-fPIC", "-pthread", "-Wall", "-Wno-sign-compare"]
    if sanitize:
        flags = ["-O1", "-g", "-std=c++17", "-fPIC", "-pthread", f"-fsanitize={sanitize}",
                 "-fno-omit-frame-pointer"]
    objs, cmds = [], []
    for s in CPU_SOURCES:
        src = EDIR / s
        obj = BUILD / (f"cpu{suffix}_" + s + ".o")
        objs.append(obj)
        if force or _newer(src, obj, headers):
            cmds.append([CXX, *flags, *(_pybind_includes()), "-c", str(src), "-o", str(obj)])
    with cf.ThreadPoolExecutor(max_workers=jobs) as ex:
        list(ex.map(_run, cmds))
    if force or cmds or not target.exists():
        link = [CXX, "-shared", "-pthread", "-o", str(target), *map(str, objs)]
        if sanitize:
            link.insert(1, f"-fsanitize={sanitize}")
        _run(link)
    return target


def build_comm(force: bool = False) -> Path:
    """_dgcomm: native RCCL communicator (host code; links librccl.so.1 — at run time the copy
    torch already mapped, same SONAME)."""
    BUILD.mkdir(exist_ok=True)
    OUT.mkdir(exist_ok=True)
    target = OUT / f"_dgcomm{EXT}"
    src = CDIR / "comm.cpp"
    kern = CDIR / "oneshot.hip"       # the one-shot IPC all-reduce kernel (small buckets)
    obj = BUILD / "comm_oneshot.hip.o"
    if force or _newer(kern, obj):
        _run([HIPCC, "-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-c", str(kern),
              "-o", str(obj)])
    hobj = BUILD / "comm_host.cpp.o"
    if force or _newer(src, hobj):
        _run([HIPCC, "-O2", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-c",
              *(_pybind_includes()), "-I/opt/rocm/include", str(src), "-o", str(hobj)])
    if force or _newer(hobj, target) or _newer(obj, target):
        _run([HIPCC, "-shared", "-fPIC", f"--offload-arch={ARCH}", str(hobj), str(obj), "-o",
              str(target), "-L/opt/rocm/lib", "-lrccl", "-lamdhip64"])
    return target


def build_all(force: bool = False) -> None:
    build_cpu(force)
    build_hip(force)
    build_smalls(SMALL, force)
    build_comm(force)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--force", action="store_true")
    ap.add_argument("--only", choices=["hip", *SMALL, "cpu", "comm"])
    ap.add_argument("--sanitize", choices=["thread", "address", "address,undefined"])
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 4))
    a = ap.parse_args(argv)

    def wanted(name):
        return a.only in (None, name)

    if wanted("cpu"):
        print(build_cpu(a.force, a.j, a.sanitize))
    if a.sanitize:
        return
    if wanted("hip"):
        print(build_hip(a.force, a.j))
    for target in build_smalls([n for n in SMALL if wanted(n)], a.force, a.j):
        print(target)
    if wanted("comm"):
        print(build_comm(a.force))


if __name__ == "__main__":
    main()
