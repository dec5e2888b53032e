"""Which kernels a call launches that brings channel IQ rows as its input (FMD_IN_CIQ_*), without a GPU: the host
objects of the library (csrc/fmd_batch.o, csrc/fmd_ciq_in.o) linked with the recording double of the HIP runtime
(tests/cpp/call_trace/hip_recorder.cpp, unchanged) and a driver of its own (tests/cpp/ciq_in_trace.cpp).  In every
scenario -- concurrency 0, 1, 2, profiling levels 1 and 2, the shared and the whole-CU serial stage -- an IQ call is
followed by a call with float rows, one with int16 rows and another IQ call, all of the same baseband length:

  - a channel IQ call launches k_ciq_in of its format once, on the stream the IQ call's IF FIR goes to, with one
    workgroup row per channel, and no k_if_* kernel: no tuner, no FIR, no level meter;
  - everything else it launches is what the IQ call of that length launches, kernel for kernel, stream for stream;
  - an IQ call launches no k_ciq_in."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pvr.rtl.radiofm_amd", "csrc")
HERE = os.path.join(ROOT, "tests", "cpp")


def _trace(workdir):
    out = subprocess.run(["make", "-C", CSRC, "fmd_batch.o", "fmd_ciq_in.o"], capture_output=True, text=True,
                         timeout=1800)
    assert out.returncode == 0, out.stderr[-3000:]  # (nothing to do where the objects are newer than csrc/)
    exe = os.path.join(workdir, "ciq_in_trace")
    cmd = ["g++", "-std=c++17", "-O1", "-w", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "call_trace", "hip_recorder.cpp"),
           os.path.join(HERE, "ciq_in_trace.cpp"), os.path.join(CSRC, "fmd_batch.o"),
           os.path.join(CSRC, "fmd_ciq_in.o"), "-o", exe, "-lpthread"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    return out.stdout


def _launches(lines):
    """(stream, kernel, grid) of every launch line"""
    out = []
    for l in lines:
        m = re.match(r"x?launch (s\d+) (.+?) grid (\S+) block", l)
        if m:
            out.append(m.groups())
    return out


def test_a_channel_iq_call_launches_the_copy_and_no_if_kernel(tmp_path):
    text = _trace(str(tmp_path))
    scenarios = text.split("== ")[1:]
    assert len(scenarios) == 5
    for block in scenarios:
        lines = block.splitlines()
        name, C = lines[0], int(re.match(r"C=(\d+)", lines[0]).group(1))
        marks = [i for i, l in enumerate(lines) if l.startswith("-- ")]
        calls = [(lines[a].split()[2], _launches(lines[a + 1:b])) for a, b in zip(marks, marks[1:])]
        assert [k for k, _ in calls] == ["iq", "ciq_f32", "ciq_s16", "iq"], name
        iq = calls[0][1]
        fir = [x for x in iq if x[1].startswith("k_if_fir")]
        assert len(fir) == 1 and len([x for x in iq if x[1].startswith("k_if_level")]) == 1, name
        rest_of_iq = [(s, k) for s, k, _ in iq if not k.startswith("k_if_")]
        for kind, launches in calls:
            if kind == "iq":
                assert not [x for x in launches if "k_ciq_in" in x[1]], (name, kind)
                assert [(s, k) for s, k, _ in launches if not k.startswith("k_if_")] == rest_of_iq, (name, kind)
                continue
            assert not [x for x in launches if x[1].startswith("k_if_")], (name, kind)
            copy = [x for x in launches if x[1].startswith("k_ciq_in")]
            want = "k_ciq_in<InCiqS16>" if kind == "ciq_s16" else "k_ciq_in<InCiqF32>"
            tiles = -(-5958 // (256 * (4 if kind == "ciq_s16" else 2)))
            assert copy == [(fir[0][0], want, "%d,%d" % (C, tiles))], (name, kind, copy)
            assert launches[0] == copy[0], (name, kind)  # in the IF stage's place: the call's first kernel
            assert [(s, k) for s, k, _ in launches if not k.startswith("k_ciq_in")] == rest_of_iq, (name, kind)
