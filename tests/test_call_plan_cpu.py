"""The position plan of a call (csrc/fmd_call_plan.hpp: baseband length M, RDS-rate samples R, audio frames A of every
call, from the positions the call before left) against the oracle's own block lengths, and its size refusals.  A
stand-alone program (tests/cpp/call_plan_check.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer walks three
geometries through a sequence of ragged call sizes; the oracle decodes all-zero blocks of the same sizes, and its
n_demod, n_rds, n_audio (fmo_get_taps) and returned audio length have to be the plan's, integer for integer."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from __graft_entry__ import ROOT
from oracle import oracle_py

SIZES = [8192, 20001, 8193, 65536, 12001, 88, 89, 30001, 8192, 9001, 176, 65535]
# IF rate, D, PCM rate, smallest call of the sequence (the program's table, in its order)
GEOMETRIES = [(2.4e6, 11, 48000.0, 0), (2.4e6, 11, 44100.0, 0), (1.0e6, 4, 48000.0, 176)]
FMD_OK, FMD_ERR_SIZE = 0, -3


@pytest.fixture(scope="module")
def plan_lines(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("call_plan") / "call_plan_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                            os.path.join(ROOT, "tests", "cpp", "call_plan_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    if build.returncode != 0 and "asan" in build.stderr.lower():
        pytest.skip("the sanitizer runtimes are not installed")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not run.stderr.strip(), run.stdout + run.stderr
    return [line.split(None, 3) if line.startswith("refusal") else line.split() for line in run.stdout.splitlines()]


def test_plan_lengths_are_the_oracles(plan_lines):
    plans = [[int(v) for v in w[1:]] for w in plan_lines if w[0] == "plan"]
    assert len(plans) == 34
    k = 0
    for g, (fs, D, pcm, smallest) in enumerate(GEOMETRIES):
        ref = oracle_py.OracleDecoder(fs, -0.15 * fs, pcm, 15000.0, D)
        for n in SIZES:
            if n < smallest:
                continue
            audio = ref.process_stream(np.zeros(2 * n, np.float32))
            t = oracle_py.FmoTaps()
            oracle_py.lib().fmo_get_taps(ref._h, oracle_py.C.byref(t))
            want = [g, n, FMD_OK, int(t.n_demod), int(t.n_rds), int(t.n_audio)]
            print("geometry %d, %5d samples: plan M R A %s, oracle %s, audio floats %d"
                  % (g, n, plans[k][3:], want[3:], audio.size))
            assert plans[k] == want
            assert audio.size == 2 * plans[k][5]
            k += 1
        ref.close()
    assert k == len(plans)


def test_every_size_refusal_has_its_code(plan_lines):
    refusals = [w for w in plan_lines if w[0] == "refusal"]
    words = ["decimator phase", "RDS rate", "32768", "CIC", "11-tap", "no audio frame"]
    assert [int(w[1]) for w in refusals] == [0, 1, 65536, 1001, 76, 550]
    for w, word in zip(refusals, words):
        assert int(w[2]) == FMD_ERR_SIZE and word in w[3], w
