#!/usr/bin/env python3
"""The vector-memory loads, stores and vmcnt waits of k_assemble_cubes' loops,
read from the compiled code (CPU only: no GPU is needed to compile to ISA).

  python tools/loop_waits.py [--all] [--keep FILE.s] [--asm FILE.s] [EXTRA flags...]

Compiles arcanefem_amd/csrc/cubes.hip with the Makefile's flags plus
`--cuda-device-only -S` (about 20 s) and, for each k_assemble_cubes instance,
prints its VGPR / LDS / scratch sizes and, for every loop that issues a global
store, the global loads, global stores and `s_waitcnt vmcnt(N)` in program
order.

Why: loads and stores share vmcnt and retire in order.  The walk stages the
next layer's coordinates (loaded before the cubes) at the loop tail, after the
flush's stores, so that wait leaves the layer's stores in flight only when it
is vmcnt(N) with N >= the stores issued since the load.  Each wait is annotated
with the stores issued since the loop's last load (at the loop's first
instructions: those of the trip before): `ok` when N is at least that many, `COVERS k` when the wait also waits for k of those stores (k = all
of them for vmcnt(0): the drain this tool exists to show).  Without --all
only the instances the library dispatches by default are printed (the headline,
RHS-add, no-RHS and staged canonical ones); the exit status is 1 if one of
those has a COVERS wait or scratch.
"""
from __future__ import annotations

import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arcanefem_amd", "csrc")

NAME = re.compile(r"k_assemble_cubesILi(\d+)ELb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)ELi(\d+)EEE")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^\s+s_c?branch\S*\s+(\.LBB\d+_\d+)")
VMCNT = re.compile(r"s_waitcnt.*vmcnt\((\d+)\)")


def makefile_flags() -> list[str]:
    """CXXFLAGS of csrc/Makefile (EXTRA empty), so the ISA is the library's."""
    arch = "gfx950"
    flags = None
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(r"ARCH \?= (\S+)", line)
        if m:
            arch = m.group(1)
        m = re.match(r"CXXFLAGS = (.*)", line)
        if m:
            flags = m.group(1)
    assert flags, "CXXFLAGS not found in the Makefile"
    flags = flags.replace("$(EXTRA)", "").replace("$(ARCH)", arch)
    return flags.split()


def compile_isa(out: str, extra: list[str]) -> None:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, *extra, *makefile_flags(), "-x", "hip", "--cuda-device-only", "-S", "cubes.hip", "-o", out]
    r = subprocess.run(cmd, cwd=CSRC, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        raise SystemExit(r.returncode)


def describe(m: re.Match) -> str:
    stride, carry, xex, yex, canon, has_rhs, rhs_add, v = (int(x) for x in m.groups())
    kind = ("staged canonical" if v & 1024 else "canonical") if canon else "box"
    rhs = "RHS add" if rhs_add else ("RHS set" if has_rhs else "no RHS")
    return f"<{stride}, carry={carry} xex={xex} yex={yex}, {kind}, {rhs}, V={v}>"


def functions(lines: list[str]):
    """(mangled name, first line, last line) of each k_assemble_cubes instance."""
    start = None
    for i, ln in enumerate(lines):
        if start is None:
            m = re.match(r"^(_Z\S*k_assemble_cubes\S*):", ln)
            if m:
                start = (m.group(1), i)
        elif ln.startswith(".Lfunc_end"):
            yield start[0], start[1], i
            start = None


def info(lines: list[str], end: int) -> dict:
    d = {}
    for ln in lines[end:end + 60]:
        for key, pat in (("vgpr", r"; NumVgprs: (\d+)"), ("agpr", r"; NumAgprs: (\d+)"),
                         ("scratch", r"; ScratchSize: (\d+)"), ("lds", r"; LDSByteSize: (\d+)"),
                         ("occupancy", r"; Occupancy: (\d+)"), ("code", r"; codeLenInByte = (\d+)")):
            m = re.match(pat, ln)
            if m and key not in d:
                d[key] = int(m.group(1))
    return d


def is_code(ln: str) -> bool:
    return ln.startswith("\t") and bool(ln.split()) and not ln.split()[0].startswith((".", ";"))


def loops(lines: list[str], lo: int, hi: int):
    """The natural loops of the kernel's control-flow graph, as (head line, sorted
    list of (first, last) line ranges of the loop's basic blocks).  A branch back
    to a label above it is a loop only if the label's block dominates it: blocks
    the compiler places out of line and that jump back to their join are not."""
    code = [i for i in range(lo, hi) if is_code(lines[i]) or LABEL.match(lines[i])]
    leaders = set()
    prev_term = True
    for i in code:
        if LABEL.match(lines[i]) or prev_term:
            leaders.add(i)
        prev_term = is_code(lines[i]) and lines[i].split()[0].startswith(("s_branch", "s_cbranch", "s_endpgm", "s_setpc"))
    starts = sorted(leaders)
    blocks = []  # (first, last)
    for k, st in enumerate(starts):
        en = (starts[k + 1] if k + 1 < len(starts) else hi) - 1
        blocks.append((st, en))
    at = {}  # label -> block
    for k, (st, en) in enumerate(blocks):
        m = LABEL.match(lines[st])
        if m:
            at[m.group(1)] = k
    succ = [[] for _ in blocks]
    for k, (st, en) in enumerate(blocks):
        last = next((i for i in range(en, st - 1, -1) if is_code(lines[i])), None)
        op = lines[last].split()[0] if last is not None else ""
        m = BRANCH.match(lines[last]) if last is not None else None
        if m and m.group(1) in at:
            succ[k].append(at[m.group(1)])
        if not op.startswith(("s_branch", "s_endpgm", "s_setpc")) and k + 1 < len(blocks):
            succ[k].append(k + 1)
    n = len(blocks)
    pred = [[] for _ in range(n)]
    for k in range(n):
        for j in succ[k]:
            pred[j].append(k)
    dom = [set(range(n)) for _ in range(n)]
    dom[0] = {0}
    changed = True
    while changed:
        changed = False
        for k in range(1, n):
            ps = [dom[p] for p in pred[k]]
            d = (set.intersection(*ps) if ps else set()) | {k}
            if d != dom[k]:
                dom[k] = d
                changed = True
    body = {}  # head -> blocks
    for t in range(n):
        for h in succ[t]:
            if h in dom[t]:
                b = body.setdefault(h, {h})
                work = [t]
                while work:
                    x = work.pop()
                    if x not in b:
                        b.add(x)
                        work.extend(pred[x])
    return [(blocks[h][0], [blocks[k] for k in sorted(b)]) for h, b in sorted(body.items())]


def is_load(op: str) -> bool:
    return op.startswith(("global_load", "flat_load", "buffer_load"))


def is_store(op: str) -> bool:
    return op.startswith(("global_store", "flat_store", "buffer_store", "global_atomic"))


def report(lines: list[str], name: str, lo: int, hi: int, out) -> bool:
    m = NAME.search(name)
    inf = info(lines, hi)
    out(f"== k_assemble_cubes{describe(m)}")
    out(f"   VGPRs {inf.get('vgpr')} (+{inf.get('agpr')} AGPRs)  LDS {inf.get('lds')} B  scratch {inf.get('scratch')} B  "
        f"occupancy {inf.get('occupancy')}  code {inf.get('code')} B")
    bad = inf.get("scratch", 0) != 0 and int(m.group(1)) == 64
    def ops(ranges):
        for a, b in ranges:
            for i in range(a, b + 1):
                if is_code(lines[i]):
                    yield i, lines[i].split()[0]

    ls = [(h, rs) for h, rs in loops(lines, lo, hi) if any(is_store(op) for _, op in ops(rs))]
    for h, rs in ls:
        inner = [r for g, r in ls if g != h and set(r) < set(rs)]
        own = [r for r in rs if not any(r in x for x in inner)]
        n_st = n_ld = 0
        # stores since the last load: at the loop's first instruction, those of the trip before
        since = 0
        for _, op in ops(own):
            since = 0 if is_load(op) else since + (1 if is_store(op) else 0)
        out(f"   loop {LABEL.match(lines[h]).group(1)} ({len(rs)} block(s), lines {rs[0][0] + 1 - lo}..{rs[-1][1] + 1 - lo} "
            "of the kernel" + (f"; the {len(inner)} loop(s) inside it are listed on their own" if inner else "") + ")")
        for i, op in ops(own):
            ln = lines[i]
            if is_load(op):
                n_ld += 1
                since = 0
                out(f"      load   {op}")
            elif is_store(op):
                n_st += 1
                since += 1
                out(f"      store  {op}{' nt' if ' nt' in ln else ''}")
            else:
                w = VMCNT.search(ln)
                if w:
                    n = int(w.group(1))
                    if n >= since:
                        note = f"ok: the {since} store(s) since the last load stay in flight"
                    else:
                        note = f"COVERS {since - n} of the {since} store(s) since the last load"
                        bad = True
                    out(f"      wait   vmcnt({n})   {note}")
        kinds = collections.Counter("VALU" if op.startswith("v_") else "LDS" if op.startswith("ds_") else
                                    "SALU" if op.startswith("s_") else "other" for _, op in ops(own))
        out(f"      -- {n_ld} load(s), {n_st} store(s) per trip; instructions in the loop's blocks: "
            f"{kinds['VALU']} VALU, {kinds['LDS']} LDS, {kinds['SALU']} SALU")
    return bad


def main() -> int:
    args = sys.argv[1:]
    show_all = "--all" in args
    args = [a for a in args if a != "--all"]
    keep = asm = None
    for flag in ("--keep", "--asm"):
        if flag in args:
            k = args.index(flag)
            if flag == "--keep":
                keep = args[k + 1]
            else:
                asm = args[k + 1]
            del args[k:k + 2]
    tmp = None
    if asm is None:
        if keep:
            asm = keep
        else:
            tmp = tempfile.NamedTemporaryFile(suffix=".s", delete=False)
            tmp.close()
            asm = tmp.name
        compile_isa(asm, args)
    try:
        lines = open(asm).read().split("\n")
    finally:
        if tmp:
            os.unlink(tmp.name)
    # the default V of the library: the headline instance's (RHS set, 64 rows, all exchanges, box)
    funcs = list(functions(lines))
    vs = sorted({int(NAME.search(n).group(8)) for n, _, _ in funcs})
    print(f"# cubes.hip: {len(funcs)} k_assemble_cubes instances, V in {vs}")
    print("# flags: " + " ".join(args + makefile_flags()))
    # the default V is the one every RHS mode of the box instance is compiled with
    cnt = collections.Counter(int(NAME.search(n).group(8)) for n, _, _ in funcs
                  if NAME.search(n).group(1, 2, 3, 4, 5) == ("64", "1", "1", "1", "0"))
    vdef = max(cnt, key=lambda v: (cnt[v], v))
    bad = False
    for name, lo, hi in funcs:
        g = NAME.search(name).groups()
        default = g[:4] == ("64", "1", "1", "1") and ((g[4] == "0" and int(g[7]) == vdef)
                                                     # (the canonical instances never carry bit 4096)
                                                     or (g[4] == "1" and int(g[7]) == ((vdef & ~4096) | 1024)
                                                         and g[5] == "0"))
        if not (show_all or default):
            continue
        b = report(lines, name, lo, hi, print)
        bad = bad or (b and default)
    print("# " + ("a default instance drains stores at a wait, or has scratch" if bad else
                  "no default instance waits for its own layer's stores; no scratch"))
    return 1 if bad else 0


if __name__ == "__main__":
    raise SystemExit(main())
