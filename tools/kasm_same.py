#!/usr/bin/env python
"""Is the device code of two source trees the same?  No GPU needed.

    python tools/kasm_same.py OLD_TREE NEW_TREE [FILE.hip ...]

Compiles every csrc/kernels/*.hip and csrc/comm/*.hip of both trees (or only the files named)
to gfx950 assembly with the build's flags (kloop_report.compile_asm) and compares the text, the
``__hip_cuid_<hex>`` symbol apart (a hash of the source text).  One line per file; the exit
status is non-zero when a file differs or exists in one tree only.  For a refactor of the
kernels' helpers: identical assembly is identical behaviour and speed.
"""
import concurrent.futures as cf
import os
import re
import sys
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kloop_report import compile_asm  # noqa: E402

CUID = re.compile(r"__hip_cuid_[0-9a-f]+")
DIRS = ("csrc/kernels", "csrc/comm")


def asm(path):
    return CUID.sub("__hip_cuid_", compile_asm(path)) if path.exists() else None


def main(argv):
    if len(argv) < 2:
        sys.exit(__doc__)
    old, new = Path(argv[0]), Path(argv[1])
    rel = sorted({str(p.relative_to(t)) for t in (old, new) for d in DIRS
                  for p in (t / d).glob("*.hip") if not argv[2:] or p.name in argv[2:]})
    with cf.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 4)) as ex:
        olds = [ex.submit(asm, old / r) for r in rel]
        news = [ex.submit(asm, new / r) for r in rel]
        bad = 0
        for r, fo, fn in zip(rel, olds, news):
            o, n = fo.result(), fn.result()
            verdict = "missing" if o is None or n is None else "same" if o == n else "DIFFERENT"
            bad += verdict != "same"
            print(f"{verdict:9s} {r}  ({0 if n is None else n.count(chr(10))} lines)", flush=True)
    print(f"{len(rel) - bad} of {len(rel)} files identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
