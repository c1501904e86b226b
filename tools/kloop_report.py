"""Static report of a kernel file's MFMA loops: cross-compiles one csrc/kernels/*.hip to gfx950
assembly (deep_go_amd/_build.py's flags plus --cuda-device-only -S; no GPU needed) and prints

  * per kernel: its mangled name, VGPR / AGPR counts and VGPR spill count;
  * per basic block with at least --min-mfma (16) MFMAs: the counts of MFMA, other VALU, LDS,
    vector-memory (loads + stores) and scalar instructions, and the ordered sequence of its
    vmcnt waits, vector-memory loads and stores, barriers and MFMA runs:
      M24 = 24 MFMAs in a row, L4 = 4 loads, S1 = 1 store, w7 = s_waitcnt vmcnt(7), B = s_barrier

A basic block starts at a label and ends at a branch, so a rolled K loop's body is one block
and its counts are per iteration.  Only those instruction classes and the waits are looked at.

  python tools/kloop_report.py conv_stack2.hip [--min-mfma 16] [--asm OUT.s] [-D NAME[=V]]...
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep_go_amd import _build  # noqa: E402

LABEL = re.compile(r"^([.\w$]+):")
INSTR = re.compile(r"^\s+([a-z_][a-z0-9_]*)\b(.*)")
VMCNT = re.compile(r"vmcnt\((\d+)\)")
BRANCH = ("s_branch", "s_cbranch", "s_endpgm", "s_setpc", "s_swappc")
VMEM = ("global_", "buffer_", "flat_", "scratch_")


def compile_asm(src, defines=()):
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        cmd = [_build.HIPCC, *_build.HIP_FLAGS, *[f"-D{d}" for d in defines],
               "--cuda-device-only", "-S", str(src), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"compile failed: {' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
        with open(out) as f:
            return f.read()


def waitcnt_vm(ops):
    """vmcnt of an s_waitcnt's operands, or None if it leaves vmcnt alone."""
    m = VMCNT.search(ops)
    if m:
        return int(m.group(1))
    ops = ops.split(";")[0].strip()
    try:
        imm = int(ops, 0)
    except ValueError:
        return None
    vm = (imm & 0xF) | ((imm >> 14) & 0x3) << 4   # gfx9 encoding: bits 3:0 and 15:14
    return None if vm == 63 else vm


class Block:
    def __init__(self, label):
        self.label = label
        self.n = dict(mfma=0, valu=0, lds=0, vmem=0, scalar=0)
        self.seq = []   # [kind, count] runs

    def push(self, kind):
        if kind[0] in "MLS" and self.seq and self.seq[-1][0] == kind:
            self.seq[-1][1] += 1
        else:
            self.seq.append([kind, 1])

    def add(self, op, ops):
        if op.startswith("v_mfma") or op.startswith("v_smfmac"):
            self.n["mfma"] += 1
            self.push("M")
        elif op.startswith("v_"):
            self.n["valu"] += 1
        elif op.startswith("ds_"):
            self.n["lds"] += 1
        elif op.startswith(VMEM):
            self.n["vmem"] += 1
            self.push("L" if "_load" in op else "S")
        elif op.startswith("s_"):
            self.n["scalar"] += 1
            if op == "s_waitcnt":
                vm = waitcnt_vm(ops)
                if vm is not None:
                    self.push(f"w{vm}")
            elif op == "s_barrier":
                self.push("B")

    def sequence(self):
        return " ".join(f"{k}{c}" if k in "MLS" else k for k, c in self.seq)


def parse(asm):
    """-> ([(kernel name, [Block])], {kernel name: metadata dict})"""
    kernels, cur, blk = [], None, None
    types = set(re.findall(r"^\s+\.type\s+([.\w$]+),@function", asm, re.M))
    for line in asm.splitlines():
        m = LABEL.match(line)
        if m:
            if m.group(1) in types:
                cur = (m.group(1), [])
                kernels.append(cur)
            if cur is not None:
                blk = Block(m.group(1))
                cur[1].append(blk)
            continue
        if cur is None or line.lstrip().startswith((";", ".")):
            if line.lstrip().startswith(".size") or line.startswith(".Lfunc_end"):
                cur = None
            continue
        m = INSTR.match(line)
        if not m:
            continue
        op, ops = m.group(1), m.group(2)
        blk.add(op, ops)
        if op.startswith(BRANCH):
            blk = Block(blk.label + "+")
            cur[1].append(blk)
    meta = {}
    for ent in re.split(r"^\s+- (?=\.)", asm, flags=re.M):
        name = re.search(r"^\s*\.name:\s+([.\w$]+)\s*$", ent, re.M)
        if not name or ".vgpr_count" not in ent:
            continue
        meta[name.group(1)] = {k: int(v) for k, v in re.findall(
            r"\.(vgpr_count|agpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", ent)}
    return kernels, meta


def report(asm, min_mfma=16, out=sys.stdout):
    kernels, meta = parse(asm)
    for name, blocks in kernels:
        md = meta.get(name, {})
        print(f"kernel {name}", file=out)
        print(f"  vgpr {md.get('vgpr_count', '?')} agpr {md.get('agpr_count', '?')} "
              f"vgpr_spills {md.get('vgpr_spill_count', '?')} "
              f"scratch_bytes {md.get('private_segment_fixed_size', '?')}", file=out)
        for b in blocks:
            if b.n["mfma"] < min_mfma:
                continue
            n = b.n
            print(f"  block {b.label}: mfma {n['mfma']} valu {n['valu']} lds {n['lds']} "
                  f"vmem {n['vmem']} scalar {n['scalar']}", file=out)
            print(f"    {b.sequence()}", file=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("source", help="a .hip file (a bare name is looked up in csrc/kernels)")
    ap.add_argument("--min-mfma", type=int, default=16)
    ap.add_argument("--asm", help="also keep the assembly here")
    ap.add_argument("-D", action="append", default=[], dest="defines")
    a = ap.parse_args()
    src = a.source if os.path.exists(a.source) else str(_build.KDIR / a.source)
    asm = compile_asm(src, a.defines)
    if a.asm:
        with open(a.asm, "w") as f:
            f.write(asm)
    report(asm, a.min_mfma)


if __name__ == "__main__":
    main()
