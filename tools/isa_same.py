#!/usr/bin/env python3
"""Whether two builds of the library's gfx950 code run the same kernels, instruction for instruction.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC --offload-device-only \\
          -c pvr.rtl.radiofm_amd/csrc/fmd_batch.hip -o new.co          (and the same at the parent commit: old.co)
    python tools/isa_same.py old.co new.co

Every kernel of OLD must have a body in NEW that is identical up to the PC-relative offsets of global tables (the
s_add_u32 / s_addc_u32 pair behind s_getpc_b64 moves with the code object's layout).  For the capture map's
kernels (template argument MAP = true) it also prints how many instructions differ from
the same kernel's default form and whether its tap loops (the innermost loops that read LDS) are the default
form's, opcode for opcode."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def disassemble(co):
    with tempfile.TemporaryDirectory() as tmp:
        elf = os.path.join(tmp, "dev.elf")
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                               "--input=" + co, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + elf])
        text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn",
                                        "--no-leading-addr", elf], text=True)
    funcs, addrs, cur, since_getpc = {}, {}, None, 99
    for line in text.splitlines():
        m = re.match(r"^<(\S+)>:$", line.strip())
        if m:
            cur = m.group(1)
            funcs[cur], addrs[cur] = [], []
            continue
        a = re.search(r"//\s*([0-9A-Fa-f]+):", line)
        t = re.sub(r"\s*//.*$", "", line.strip())
        if not cur or not t:
            continue
        since_getpc = 0 if t.startswith("s_getpc_b64") else since_getpc + 1
        if since_getpc <= 2 and t.startswith(("s_add_u32", "s_addc_u32")):
            t = re.sub(r"0x[0-9a-f]+$", "<rel>", t)
        funcs[cur].append(t)
        addrs[cur].append(int(a.group(1), 16) if a else -1)
    return funcs, addrs


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, out))


def loops(body, addr):
    """index ranges of the loops: a backward branch (simm16 in dwords, relative to the next instruction)"""
    spans = []
    for i, t in enumerate(body):
        m = re.match(r"s_(?:cbranch_\w+|branch) (\d+)$", t)
        if m and addr[i] >= 0:
            off = int(m.group(1))
            off = off - 65536 if off >= 32768 else off
            if off < 0:
                tgt = addr[i] + 4 + 4 * off
                lo = next((k for k, x in enumerate(addr) if x >= tgt), i)
                spans.append((lo, i))
    return spans


def inner_loops(body, addr):
    """opcode sequences of the loops that contain no other loop"""
    spans = loops(body, addr)
    inner = [(lo, hi) for lo, hi in spans
             if not any((l2, h2) != (lo, hi) and lo <= l2 and h2 <= hi for l2, h2 in spans)]
    return [tuple(x.split()[0] for x in body[lo:hi + 1]) for lo, hi in inner]


def main(old_co, new_co):
    (old, _), (new, new_addr) = disassemble(old_co), disassemble(new_co)
    bodies = {}
    for n, v in new.items():
        bodies.setdefault("\n".join(v), []).append(n)
    bad = [n for n, v in old.items() if new.get(n) != v and "\n".join(v) not in bodies]
    names = demangle(sorted(set(old) | set(new)))
    print("kernels of the old build: %d, identical in the new one: %d" % (len(old), len(old) - len(bad)))
    for n in bad:
        print("  DIFFERS: " + names[n][:150])
    # the map forms against their default forms: the same demangled name with MAP false
    default_of = {names[n]: n for n in new}
    print("map forms (MAP = true) against the default form:")
    taps_ok = True
    for n in sorted(new):
        d = names[n]
        if not d.startswith("void fmd::k_if_") or ", true>(" not in d:
            continue
        m = re.match(r"(void fmd::k_if_\w+<.*), true>(\(.*)$", d)
        twin = default_of.get(m.group(1) + ", false>" + m.group(2)) if m else None
        if twin is None:
            continue
        a, b = new[twin], new[n]
        ops = difflib.SequenceMatcher(a=a, b=b, autojunk=False).get_opcodes()
        changed = sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in ops if tag != "equal")
        # the innermost loops' opcode sequences (register numbers may differ: the two forms allocate apart); the tap
        # loops are the ones that read the window from LDS
        la, lb = inner_loops(a, new_addr[twin]), inner_loops(b, new_addr[n])
        ta = sorted(x for x in la if any(o.startswith("ds_read") for o in x))
        tb = sorted(x for x in lb if any(o.startswith("ds_read") for o in x))
        same = sum(1 for x in lb if x in la)
        taps_ok = taps_ok and ta == tb
        print("  %-100s %5d insts (default %5d), %4d differ; tap loops the default's: %s; inner loops: %d of %d"
              % (d[:100], len(b), len(a), changed, "yes" if ta == tb else "NO", same, len(lb)))
    print("every map form's tap loops are its default form's, opcode for opcode: %s" % ("yes" if taps_ok else "NO"))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
