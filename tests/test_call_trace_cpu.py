"""The submission order of a process call, pinned without a GPU.

The host object of csrc/fmd_batch.hip is linked with a recording double of the HIP runtime
(tests/cpp/call_trace/hip_recorder.cpp: kernels are not run, every launch, event record, stream wait, copy and
synchronisation becomes a line of text) and a driver over the C ABI (tests/cpp/call_trace/call_trace.cpp: every
concurrency mode, stream layout, kernel form, entry point and edit).  The program's output, reduced per scenario to
a SHA-256 of the whole scenario (setup calls included) and the trace of the last call as text (in full, or as the
few lines in which it differs from an earlier scenario's), has to equal tests/golden/call_trace.txt byte for byte.
The golden was recorded from the csrc/ of the commit in front of the one that split the call path into stages and schedules, and is the record of which kernel goes to which stream behind
which event: a change of the submission order shows up here as a readable diff, and is either a bug or comes with a
new golden and a GPU run.  The scenarios of the driver's parts_regions_queues (collects, the device export, state blobs
with their size and hash, the settings a shell mirrors) were added to it from the csrc/ of the commit in front of the
one that brought parts(), carried_regions() and drain_queues(): lines added, none changed.

What is not pinned: kernel arguments (which buffer a launch gets) -- the bit-exact GPU tests hold those.

To record a golden from any checkout (an object built with `make -C pvr.rtl.radiofm_amd/csrc fmd_batch.o`):
    python tests/test_call_trace_cpu.py path/to/fmd_batch.o > tests/golden/call_trace.txt
No LD_PRELOAD, no sanitizer: the double is linked in, and the process never opens a GPU wherever it runs."""
import difflib
import hashlib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pvr.rtl.radiofm_amd", "csrc")
HERE = os.path.join(ROOT, "tests", "cpp", "call_trace")
GOLDEN = os.path.join(ROOT, "tests", "golden", "call_trace.txt")


def build_and_run(obj, workdir):
    exe = os.path.join(workdir, "call_trace")
    cmd = ["g++", "-std=c++17", "-O1", "-w", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "hip_recorder.cpp"),
           os.path.join(HERE, "call_trace.cpp"), obj, "-o", exe, "-lpthread"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    return out.stdout


def _sha(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def _renumber_events(lines):
    """Events named in the order in which the lines first mention them (e0, no event, stays): which slot of the
    rotation a call has does not show in its text -- the hash over the real numbers pins that -- and calls with the
    same schedule read the same."""
    names = {"e0": "e0"}
    return [re.sub(r"\be\d+\b", lambda m: names.setdefault(m.group(0), "e%d" % len(names)), l) for l in lines]


def _delta(base, text):
    """text as an edit of base: per changed place the 1-based line of base, how many of its lines go (a single line
    that is replaced by one: the line itself, "- ") and the lines that come ("+ ")."""
    out = []
    for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, base, text, autojunk=False).get_opcodes():
        if tag != "equal":
            one = i2 - i1 == 1 and j2 - j1 == 1
            out.append("@ line %d" % (i1 + 1) + ("" if one or i2 == i1 else ", %d lines go" % (i2 - i1)))
            out += (["- " + base[i1]] if one else []) + ["+ " + l for l in text[j1:j2]]
    return out


def _kernel_list(names):
    """The sorted kernel list; instances that differ only in the input format (the first template argument, In*) share
    a line: k<{InF32,InU8}, 64> stands for k<InF32, 64> and k<InU8, 64>."""
    groups = {}
    for n in names:
        m = re.match(r"(\w+<)(In\w+)(, .*|>)$", n)
        key = (m.group(1), m.group(3)) if m else (n, "")
        groups.setdefault(key, []).append(m.group(2) if m else "")
    return sorted("kernel " + (a + "{" + ",".join(sorted(f)) + "}" + z if f != [""] else a) for (a, z), f in groups.items())


def reduce_trace(text):
    """Per scenario ("== name" up to the next one): the header, the SHA-256 and line count of all of it (setup calls
    included) and the lines from the last "-- call" on, their events renumbered (_renumber_events) -- in full, or, where that is shorter, as an edit (_delta) of
    the earlier scenario whose last call is closest.  The kernel list once (_kernel_list), with the SHA-256 of the
    mangled names."""
    out, seen = [], []
    for block in text.split("== ")[1:]:
        lines = block.splitlines()
        out.append("== " + lines[0])
        body = lines[1:]
        calls = [i for i, l in enumerate(body) if l.startswith("-- call")]
        if calls:
            out.append("sha256 %s of %d lines, %d calls" % (_sha(body), len(body), len(calls)))
            last = _renumber_events(body[calls[-1]:])
            best = min(((len(d), k, d) for k, d in enumerate(_delta(t, last) for _, t in seen)), default=None)
            if best and best[0] + 1 < len(last):
                out.append("last call as in '%s'%s" % (seen[best[1]][0], " but" if best[2] else ""))
                out.extend(best[2])
            else:
                out.extend(last)
            seen.append((lines[0], last))
            continue
        out.extend(_kernel_list([l[7:] for l in body if l.startswith("kernel ")]))
        names = [l for l in body if l.startswith("mangled ")]
        out.append("sha256 %s of %d mangled names" % (_sha(names), len(names)))
    return "\n".join(out) + "\n"


def test_submission_order_equals_the_recorded_one(tmp_path):
    obj = os.path.join(CSRC, "fmd_batch.o")
    out = subprocess.run(["make", "-C", CSRC, "fmd_batch.o"], capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0, out.stderr[-3000:]  # (nothing to do where the object is newer than csrc/)
    raw = build_and_run(obj, str(tmp_path))
    got = reduce_trace(raw)
    with open(GOLDEN) as f:
        want = f.read()
    if got != want:
        g, w = got.splitlines(), want.splitlines()
        first = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
        header = next((l for l in reversed(w[:first + 1]) if l.startswith("== ")), "?")
        (tmp_path / "call_trace_got.txt").write_text(got)
        (tmp_path / "call_trace_complete.txt").write_text(raw)
        raise AssertionError("the trace differs from tests/golden/call_trace.txt at line %d, in scenario %r:\n"
                             "  recorded: %s\n  now:      %s\n(in %s: call_trace_got.txt, what the golden would be "
                             "now, and call_trace_complete.txt, every runtime call of every scenario)"
                             % (first + 1, header, w[first] if first < len(w) else "<end>",
                                g[first] if first < len(g) else "<end>", tmp_path))


if __name__ == "__main__":
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        sys.stdout.write(reduce_trace(build_and_run(sys.argv[1], d)))
