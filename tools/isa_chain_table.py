#!/usr/bin/env python3
"""Instruction count of the half-band chain's step loop (k_halfband_chain), by class, from the ISA hipcc emits
for gfx950.  The kernel is bound by instruction issue (docs/MEASUREMENTS.md), so the count of this loop is its
cost model: instructions per step x steps x waves / SIMDs x cycles per instruction.

    python tools/isa_chain_table.py [--csrc DIR] [--form 7,11,21,true] [extra hipcc flags ...]

--csrc: the directory of fmd_k_rds.hip.h to compile (default: the tree's; another checkout's to compare).

The main loop is the function's largest loop (the blocks the compiler marks as its members): four steps.  Two
tables: every instruction of those blocks (the loop as it lies in memory, rare paths included), and the COMMON
PATH through it -- a walk from the loop's head to its back edge that takes, at every forward conditional branch,
the successor that keeps all of a step's packed arithmetic on the way and otherwise issues fewer instructions (a
rare path -- a tail, a masked ring slot -- is a detour that rejoins the stream; a stage skipped by a wave without
outputs is not what the table is about).  Where the loop holds several equal variants
of one block (the ring reads: one per place of the wrap), the walk passes through one of them, which is what a
wave does."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = os.path.join(ROOT, "tools", "ubench", "halfband_chain_isa.hip")
CLASSES = ["packed FP32 arithmetic (v_pk_mul_f32 / v_pk_add_f32)", "scalar ALU", "s_waitcnt / s_nop",
           "v_readlane_b32 / v_writelane_b32", "other VALU", "LDS", "global loads / stores", "s_load", "branches",
           "barriers"]


def classify(op):
    if op.startswith(("s_nop", "s_waitcnt")):
        return CLASSES[2]
    if op.startswith("s_barrier"):
        return CLASSES[9]
    if op.startswith(("s_cbranch", "s_branch", "s_setpc", "s_swappc")):
        return CLASSES[8]
    if op.startswith(("s_load", "s_buffer_load")):
        return CLASSES[7]
    if op.startswith("s_"):
        return CLASSES[1]
    if op.startswith("ds_"):
        return CLASSES[5]
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return CLASSES[6]
    if op.startswith(("v_readlane", "v_writelane")):
        return CLASSES[3]
    if op.startswith(("v_pk_mul_f32", "v_pk_add_f32", "v_pk_fma_f32")):
        return CLASSES[0]
    return CLASSES[4]


def compile_unit(csrc, flags):
    with tempfile.TemporaryDirectory() as td:
        asm = os.path.join(td, "k.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
                               "-ffp-contract=off", "-S", "--cuda-device-only", "-I", csrc, UNIT, "-o", asm] + flags,
                              stderr=subprocess.DEVNULL)
        return open(asm).read().splitlines()


def function(text, form):
    h0, h1, h2, osc = form
    pat = re.compile(r"^_ZN3fmd16k_halfband_chainILi%sELi%sELi%sELb%dEE\w*:" % (h0, h1, h2, osc == "true"))
    start = next(i for i, l in enumerate(text) if pat.match(l))
    end = next(i for i in range(start, len(text)) if text[i].strip().startswith(".Lfunc_end"))
    meta = {}
    for l in text[end:]:
        m = re.match(r"^; (NumSgprs|NumVgprs|NumAgprs|ScratchSize|Occupancy|LDSByteSize|SGPRBlocks)?(.*?): (\d+)", l)
        if m and (m.group(1) or m.group(2)) not in meta:
            meta[m.group(1) or m.group(2)] = int(m.group(3))
        if l.startswith("_ZN3fmd") or len(meta) > 40:
            break
    return text[start:end], meta


def parse(fn):
    """[(opcode, branch target or None, header label of the innermost loop the block lies in or None)]; labels"""
    ins, labels, pending, loop = [], {}, [], None
    for l in fn:
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
        ins.append((m.group(1), t.group(1) if t else None, loop))
    return ins, labels


def main_loop(ins, labels):
    """header label of the loop with the most instructions, and the indices of its instructions"""
    cnt = collections.Counter(x[2] for x in ins if x[2])
    head = cnt.most_common(1)[0][0]
    return head, [i for i, x in enumerate(ins) if x[2] == head]


def table(title, ops, steps):
    cnt = collections.Counter(classify(o) for o in ops)
    print("\n%s: %d instructions per %d steps = %.0f per step" % (title, len(ops), steps, len(ops) / steps))
    print("  | class | instructions per %d steps |\n  |---|---|" % steps)
    for k in CLASSES:
        print("  | %s | %d |" % (k, cnt.get(k, 0)))
    print("  | **total** | **%d** |" % len(ops))


def main():
    args, csrc, form = sys.argv[1:], os.path.join(ROOT, "pvr.rtl.radiofm_amd", "csrc"), "7,11,21,true"
    while args and args[0] in ("--csrc", "--form"):
        if args[0] == "--csrc":
            csrc = args[1]
        else:
            form = args[1]
        args = args[2:]
    fn, meta = function(compile_unit(csrc, args), form.split(","))
    ins, labels = parse(fn)
    head, member = main_loop(ins, labels)
    print("k_halfband_chain<%s> of %s" % (form, csrc))
    print("registers and occupancy: " + ", ".join("%s %d" % kv for kv in meta.items()
                                                   if kv[0] in ("NumSgprs", "NumVgprs", "ScratchSize", "Occupancy",
                                                                "LDSByteSize")))
    steps = 4
    table("main loop, all of its blocks", [ins[i][0] for i in member], steps)
    path = full_path(ins, labels, head, member)
    table("main loop, common path of a wave with outputs in every stage", [ins[i][0] for i in path], steps)
    lanes = sum(ins[i][0].startswith(("v_readlane", "v_writelane")) for i in member)
    print("\nv_readlane_b32 / v_writelane_b32 anywhere in the loop: %d" % lanes)


def full_path(ins, labels, head, member):
    """The cheapest path from the loop's head to a back edge among those with the most packed arithmetic: the path
    of least (-packed, instructions) over the loop's control flow without its back edges, which is acyclic (the
    step loop holds no inner loop; the block layout may still jump backwards to a join), by depth-first search
    with memory."""
    lo, inside, END = labels[head], set(member), -1

    def succ(i):
        op, tgt = ins[i][:2]
        if op.startswith("s_branch") and tgt:
            nxt = [labels[tgt]]
        else:
            nxt = [i + 1] + ([labels[tgt]] if op.startswith("s_cbranch") and tgt else [])
        return [END if n == lo else n for n in nxt if n in inside]

    def own(i):
        return (-1 if classify(ins[i][0]) == CLASSES[0] else 0, 1)

    memo, state, stack = {END: ((0, 0), None)}, {}, [lo]
    while stack:
        i = stack[-1]
        if i in memo:
            stack.pop()
            continue
        nxt = succ(i)
        todo = [n for n in nxt if n not in memo]
        if todo:
            if any(state.get(n) == 1 for n in todo):
                sys.exit("the step loop holds an inner loop: no single path through it")
            state[i] = 1
            stack.extend(todo)
            continue
        state[i] = 2
        stack.pop()
        if not nxt:  # a way out of the loop: not a path to the back edge
            memo[i] = ((0, 1 << 60), None)
            continue
        n = min(nxt, key=lambda k: memo[k][0])
        memo[i] = ((memo[n][0][0] + own(i)[0], memo[n][0][1] + own(i)[1]), n)
    path, i = [], lo
    while i != END:
        path.append(i)
        i = memo[i][1]
    return path


if __name__ == "__main__":
    main()
