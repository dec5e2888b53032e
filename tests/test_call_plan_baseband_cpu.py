"""The position plan of a call that brings its baseband itself (csrc/fmd_call_plan.hpp, plan_call_baseband: channel IQ
rows as a call's input, FMD_IN_CIQ_*) against the plan of the IQ call that produces the same baseband length.  A
stand-alone program (tests/cpp/call_plan_baseband_check.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer walks
five geometries -- the three of tests/test_call_plan_cpu.py, one with CIC stages, one with the 11-tap class -- through
a stream of 3647 call sizes from 1 to 65 536 samples, each at the positions the call before left: plan_call(N) and
plan_call_baseband(M of that call) agree in code, sentence, M, R, A, every half-band stage's input count and regime,
rs_pos bit for bit and the feed's counts, and the baseband plan carries no decimator phase.  plan_call itself is held
against the oracle by tests/test_call_plan_cpu.py."""
import os
import shutil
import subprocess

import pytest

from __graft_entry__ import ROOT

FMD_OK, FMD_ERR_SIZE = 0, -3


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("call_plan_baseband") / "call_plan_baseband_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                            os.path.join(ROOT, "tests", "cpp", "call_plan_baseband_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    if build.returncode != 0 and "asan" in build.stderr.lower():
        pytest.skip("the sanitizer runtimes are not installed")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and not run.stderr.strip(), run.stdout + run.stderr
    return run.stdout.splitlines()


def test_baseband_plan_is_the_iq_plan_of_the_same_length(lines):
    assert not [l for l in lines if l.startswith("mismatch")], lines[:8]
    geo = [[int(v) for v in l.split()[1::2]] for l in lines if l.startswith("geometry")]
    assert [g[0] for g in geo] == [0, 1, 2, 3, 4]
    for g, calls, accepted, refused, bad in geo:
        print("geometry %d: %d calls, %d accepted, %d refused, %d mismatches" % (g, calls, accepted, refused, bad))
        assert calls == 3647 and accepted + refused == calls and bad == 0
        assert accepted > (1000 if g == 3 else 3000) and refused > 0  # both kinds of call were compared
    assert geo[3][3] > 1500  # the CIC geometry refuses every odd length: the same sentence from both plans


def test_every_baseband_refusal_has_its_code_and_sentence(lines):
    refusals = [l.split(None, 3) for l in lines if l.startswith("refusal")]
    assert [int(w[1]) for w in refusals] == [0, 1, 32718, 32717, 1001, 19, 50]
    words = ["no baseband samples", "RDS rate", "32768", None, "CIC", "11-tap", "no audio frame"]
    for w, word in zip(refusals, words):
        if word is None:  # M + 51 == 32768: the largest block the reference's buffers hold
            assert int(w[2]) == FMD_OK and w[3] == "-", w
        else:
            assert int(w[2]) == FMD_ERR_SIZE and word in w[3], w
