#!/usr/bin/env python3
"""What one tile of the headline IF FIR (k_if_fir_mt3) issues, by class, from the ISA hipcc emits for gfx950: the
counterpart of tools/isa_chain_table.py for the kernel that holds half the pipeline's joules.

    python tools/isa_fir_table.py [--csrc DIR] [--form InF32,12,2,2,false] [extra hipcc flags ...]

--csrc: the directory of fmd_k_if.hip.h to compile (default: the tree's; another checkout's to compare).
--form: input format, loads per lane, tiles per workgroup, outputs per lane, capture map.

The kernel holds one body per kind of tile and place in the workgroup (tools/ubench/if_fir_isa.hip is the compile
unit); the tap loops are the loops that read the window from LDS and multiply.
A body is told by the wave synchronisation that ends its staging (bodies may share their tails).  For each the tool
walks from the kernel's entry to it and on to the synchronisation that ends the tile -- at every forward
conditional branch the way with the most LDS and global operations and then the fewest instructions, never into a
loop other than a tap loop (the history, ragged-end and next-call-history loops run for a call's first and last tile
only) -- and keeps the part of the walk behind the previous tile's end: one tile as a wave with all its lanes in
range issues it, the tap loop counted as often as it runs.  A workgroup's first tile carries the kernel's prologue and
the choice between the bodies; its second tile is the tile alone.  Two parts per tile: staging (up to the
synchronisation in front of the tap loop) and everything behind it (the next tile's loads, the taps, the stores).

A limitation: the walk reads this compiler's idioms -- the flags it routes the choice between bodies through (a
64-bit scalar move, an AND with exec, a branch on vcc), "branch if any lane is active" as a jump -- and picks ways by
a rule of thumb (most memory operations, then fewest instructions).  It fits what hipcc emits for this kernel today
and gives the figures of docs/MEASUREMENTS.md; after a compiler change check its output against the ISA (the number
of bodies and of interior ones, 12 loads and 12 LDS writes per staging) before relying on it."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = os.path.join(ROOT, "tools", "ubench", "if_fir_isa.hip")
CLASSES = ["packed FP32 arithmetic", "other VALU", "LDS reads and writes", "global / buffer loads and stores",
           "scalar loads", "scalar ALU", "waits / nops", "branches"]


def classify(op):
    if op.startswith(("s_nop", "s_waitcnt")):
        return CLASSES[6]
    if op.startswith(("s_cbranch", "s_branch", "s_setpc", "s_swappc", "s_endpgm")):
        return CLASSES[7]
    if op.startswith(("s_load", "s_buffer_load")):
        return CLASSES[4]
    if op.startswith("s_"):
        return CLASSES[5]
    if op.startswith("ds_"):
        return CLASSES[2]
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return CLASSES[3]
    if op.startswith(("v_pk_mul_f32", "v_pk_add_f32", "v_pk_fma_f32")):
        return CLASSES[0]
    return CLASSES[1]


def compile_unit(csrc, flags):
    with tempfile.TemporaryDirectory() as td:
        asm = os.path.join(td, "k.s")
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
                               "-ffp-contract=off", "-S", "--cuda-device-only", "-I", csrc, UNIT, "-o", asm]
        r = subprocess.run(cmd + flags, stderr=subprocess.PIPE, text=True)
        if r.returncode:
            sys.exit("hipcc failed:\n" + r.stderr)
        return open(asm).read().splitlines()


def function(text, form):
    fmt, unroll, nt, ro, mp = form
    pat = re.compile(r"^_ZN3fmd12k_if_fir_mt3INS_%d%sELi%sELi%sELi%sELi88ELi11ELb0ELb%dEE\w*:"
                     % (len(fmt), fmt, unroll, nt, ro, mp == "true"))
    start = next(i for i, l in enumerate(text) if pat.match(l))
    end = next(i for i in range(start, len(text)) if text[i].strip().startswith(".Lfunc_end"))
    meta = {}
    for l in text[end:]:
        m = re.match(r"^; (NumSgprs|NumVgprs|ScratchSize|Occupancy): (\d+)", l)
        if m and m.group(1) not in meta:
            meta[m.group(1)] = int(m.group(2))
        if l.startswith("_ZN3fmd"):
            break
    return text[start:end], meta


def parse(fn):
    """[(opcode, branch target or None, header label of the innermost loop the block lies in or None, written as an
    asm statement, operands)]; labels"""
    ins, labels, pending, loop, in_asm = [], {}, [], None, False
    for l in fn:
        if "#ASMSTART" in l or "#ASMEND" in l:
            in_asm = "#ASMSTART" in l
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        b = m or re.match(r"^; %bb\.\d+:", l)
        if b:
            h = re.search(r"in Loop: Header=(BB\d+_\d+)", l)
            loop = ".L" + h.group(1) if h else (m.group(1) if m and "Loop Header" in l else None)
        if m:
            pending.append(m.group(1))
            continue
        m = re.match(r"^\s+([a-z]\w*)\s*(.*?)\s*(;.*)?$", l)
        if not m or l.lstrip().startswith((";", ".")):
            continue
        for p in pending:
            labels[p] = len(ins)
        pending = []
        t = re.match(r"^(\.LBB\d+_\d+)$", m.group(2)) if m.group(1).startswith(("s_cbranch", "s_branch")) else None
        ins.append((m.group(1), t.group(1) if t else None, loop, in_asm, m.group(2)))
    return ins, labels


def tap_loops(ins):
    """the loops that read LDS and multiply: [(header label, indices of its instructions)] in the order they lie"""
    members = collections.defaultdict(list)
    for i, x in enumerate(ins):
        if x[2]:
            members[x[2]].append(i)
    out = []
    for head, idx in members.items():
        ops = [ins[i][0] for i in idx]
        if any(o.startswith("ds_read") for o in ops) and sum(classify(o) == CLASSES[0] for o in ops) >= 20:
            out.append((head, idx))
    return sorted(out, key=lambda t: t[1][0])


MEMORY = (CLASSES[2], CLASSES[3])


def walk(ins, labels, allowed_loops, start, goals, blocked=()):
    """The way from instruction `start` to the first of `goals` it meets with the most LDS and global operations and
    then the fewest instructions, over the control flow without backward branches and without the loops not in
    allowed_loops."""
    def succ(i):
        op, tgt = ins[i][:2]
        if op.startswith("s_endpgm"):
            return []
        # (the compiler routes the choice between the bodies through flags: a flag set to a constant and tested by the
        # next two instructions is a jump, or none)
        if op == "s_mov_b64" and i + 2 < len(ins) and ins[i + 2][1] and ins[i + 2][0] in ("s_cbranch_vccz",
                                                                                        "s_cbranch_vccnz"):
            reg, _, val = ins[i][4].partition(", ")
            test = ins[i + 1]
            if val in ("0", "-1") and test[0] in ("s_and_b64", "s_andn2_b64") and test[4] == "vcc, exec, " + reg:
                vcc = (val == "-1") != (test[0] == "s_andn2_b64")
                taken = vcc == (ins[i + 2][0] == "s_cbranch_vccnz")
                n = labels[ins[i + 2][1]] if taken else i + 3
                return [] if n in blocked or (ins[n][2] and ins[n][2] not in allowed_loops) else [n]
        # (outside a loop the compiler writes some jumps as "branch if any lane is active", which a running wave
        # always is: the instruction behind such a branch is another body's, not a way on)
        if tgt and (op.startswith("s_branch") or (op == "s_cbranch_execnz" and not ins[i][2])):
            nxt = [labels[tgt]]
        else:
            nxt = [i + 1] + ([labels[tgt]] if op.startswith("s_cbranch") and tgt else [])
        ok = []
        for n in nxt:
            if n >= len(ins) or n in blocked or (ins[n][2] and ins[n][2] not in allowed_loops):
                continue
            if ins[n][2] and ins[n][2] == ins[i][2] and n <= i:
                continue  # the loop's back edge
            ok.append(n)
        return ok

    def own(i):
        return -1 if classify(ins[i][0]) in MEMORY else 0

    memo, state, stack = {g: ((own(g), 1), None) for g in goals if g != start}, {}, [start]
    while stack:
        i = stack[-1]
        if i in memo:
            stack.pop()
            continue
        nxt = succ(i)
        todo = [n for n in nxt if n not in memo and state.get(n) != 1]
        if todo:
            state[i] = 1
            stack.extend(todo)
            continue
        stack.pop()
        done = [n for n in nxt if memo.get(n) is not None]
        if not done:
            memo[i] = None
            continue
        n = min(done, key=lambda k: memo[k][0])
        memo[i] = ((memo[n][0][0] + own(i), memo[n][0][1] + 1), n)
    if memo[start] is None:
        return None
    path, i = [], start
    while i is not None:
        path.append(i)
        i = memo[i][1]
    return path


def is_sync(x):
    return x[3] and x[0].startswith("s_waitcnt")


def tiles(ins, labels, trips):
    """[(kind, place, {class: [staging, rest]}, range tests in staging)] for every tile body: a body is told by the
    synchronisation that ends its staging"""
    heads = {h for h, _ in tap_loops(ins)}
    syncs = [i for i, x in enumerate(ins) if is_sync(x)]
    out = []
    def key(path):
        return (-sum(classify(ins[i][0]) in MEMORY for i in path), len(path))

    for s in syncs:
        # from the end of a tile without another synchronisation on the way: a workgroup's second tile (the compiler
        # routes the choice between the bodies through flags, so the kernel's entry reaches those too, on ways no
        # wave takes); otherwise from the kernel's entry: its first
        others = set(syncs) - {s}
        ways = [walk(ins, labels, heads, e, {s}, others - {e}) for e in others]
        ways = [w[1:] for w in ways if w]
        front, second = (min(ways, key=key), True) if ways else (walk(ins, labels, heads, 0, {s}, others), False)
        if front is None:
            continue
        back = walk(ins, labels, heads, s, set(syncs))
        if back is None or not any(ins[i][2] in heads for i in back):
            continue  # the synchronisation that ends a tile
        seg = front + back[1:]
        cut = seg.index(s)
        cnt = {k: [0, 0] for k in CLASSES}
        for pos, i in enumerate(seg):
            times = trips if ins[i][2] in heads else 1
            cnt[classify(ins[i][0])][0 if pos <= cut else 1] += times
        tests = sum(ins[i][0].startswith("s_and_saveexec") for i in seg[:cut])
        out.append(("interior" if tests <= 1 else "edge", "second" if second else "first", cnt, tests))
    return out


def window_bytes(csrc, ro):
    """The kernel's LDS is dynamic, so the ISA does not hold its size: what the launch of that checkout allocates
    (lds_l of fmd_batch_if.inc.hpp) -- the window of (64 RO - 1) D + order + 4 samples, or, where the launch takes
    them, all 12 rounds' pairs for two outputs per lane."""
    host = open(os.path.join(csrc, "fmd_batch_if.inc.hpp")).read()
    if ro == 2 and re.search(r"lds_l = RO == 2 \? size_t\(12\) \* 64 \* 2 \* sizeof\(float2\)", host):
        return 12 * 64 * 2 * 8
    return ((64 * ro - 1) * 11 + 88 + 4) * 8


def main():
    args, csrc, form = sys.argv[1:], os.path.join(ROOT, "pvr.rtl.radiofm_amd", "csrc"), "InF32,12,2,2,false"
    while args and args[0] in ("--csrc", "--form"):
        if args[0] == "--csrc":
            csrc = args[1]
        else:
            form = args[1]
        args = args[2:]
    f = form.split(",")
    fn, meta = function(compile_unit(csrc, args), f)
    ins, labels = parse(fn)
    ro = int(f[3])
    print("k_if_fir_mt3<%s> of %s" % (form, csrc))
    lds = window_bytes(csrc, ro)
    print("registers and occupancy: " + ", ".join("%s %d" % kv for kv in meta.items())
          + "; LDS (the window, allocated at the launch): %d B, %d waves per CU of 160 KB" % (lds, 160 * 1024 // lds))
    bodies = tiles(ins, labels, 8 - (ro - 1))
    print("instructions in the kernel: %d; tap loops: %d; tile bodies: %d, of them interior: %d"
          % (len(ins), len(tap_loops(ins)), len(bodies), sum(b[0] == "interior" for b in bodies)))
    seen = set()
    for kind, place, cnt, tests in bodies:
        key = (kind, place, tuple(tuple(v) for v in cnt.values()))
        if key in seen:
            continue
        seen.add(key)
        tot = [sum(v[0] for v in cnt.values()), sum(v[1] for v in cnt.values())]
        print("\n%s tile, the workgroup's %s (%d range tests in staging): %d instructions"
              % (kind, place, tests, tot[0] + tot[1]))
        print("  | class | staging | loads of the next tile, taps, stores | tile |\n  |---|---|---|---|")
        for k in CLASSES:
            print("  | %s | %d | %d | %d |" % (k, cnt[k][0], cnt[k][1], cnt[k][0] + cnt[k][1]))
        print("  | **total** | **%d** | **%d** | **%d** |" % (tot[0], tot[1], tot[0] + tot[1]))


if __name__ == "__main__":
    main()
