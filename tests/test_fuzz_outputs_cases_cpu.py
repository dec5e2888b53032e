"""Preconditions of tests/test_gpu_fuzz_outputs.py, from the generator and the CPU oracle alone: the default cases
visit every value of every axis, the streams hold what makes the comparisons bite (frame-count and M residues, feed
phases, saturation, RDS records of every status), and the RDS restatement agrees with the oracle at every drawn
geometry.  Conditions, not measurements: if one fails, the stratification or the stations change, not the bound."""
import collections

import numpy as np
import fuzz_outputs_cases as fc

_EXP = {}


def _all(oracle, fmsig):
    if not _EXP:
        for k in fc.cases(fc.N_DEFAULT):
            _EXP[k["seed"]] = (k, fc.expectations(k, oracle, fmsig))
    return [_EXP[i] for i in range(fc.N_DEFAULT)]


def test_axis_coverage(oracle):
    ks = [fc.resolve(k, oracle) for k in fc.cases(fc.N_DEFAULT)]
    n = collections.Counter()
    for k in ks:
        for key in ("pcm", "bw", "feed_div", "rds_mode", "C", "table", "edit", "mode", "lag", "loud", "u8", "us", "cic",
                    "shared"):
            n[(key, k[key])] += 1
        n[("D even", k["D"] % 2 == 0)] += 1
        n[("order >= 1000", k["order"] >= 1000)] += 1
        n[("order", k["order"])] += 1
        n[("table not 0 / 64", k["table"] not in (0, 64))] += 1
        for kind in fc.KINDS:
            n[("selection", k["sel"][kind])] += 1
        for o in k["outs"]:
            for kind in fc.KINDS:
                n[("calls " + kind, o[kind])] += 1
    for key in sorted(n, key=str):
        print("%-22s %-10s %d" % (key[0], key[1], n[key]))
    assert all(n[("pcm", v)] >= 8 for v in fc.PCM)
    assert all(n[("bw", v)] >= 8 for v in fc.BW)
    assert all(n[("feed_div", v)] >= 12 for v in (2, 3))
    assert all(n[("rds_mode", v)] >= 6 for v in (0, 1, 2))
    for kind in fc.KINDS[1:]:
        assert all(n[("calls " + kind, v)] >= 20 for v in fc.FMT), kind
    assert all(n[("calls audio", v)] >= 20 for v in ("f32", "s16"))
    for kind in fc.KINDS:  # every shape of every row kind somewhere
        assert {k["sel"][kind] for k in ks} == set(fc.SHAPES), kind
    assert n[("cic", True)] >= 2 and n[("D even", True)] >= 6 and n[("order >= 1000", True)] >= 4
    assert n[("u8", True)] >= 8 and n[("table not 0 / 64", True)] >= 10
    assert all(n[("edit", v)] >= 5 for v in fc.EDITS)
    assert all(n[("selection", v)] >= 6 for v in fc.SHAPES)
    assert all(n[("C", v)] >= 4 for v in fc.CHANNELS) and n[("C", 1030)] == 2
    assert all(n[("table", v)] >= 3 for v in fc.TABLES)
    print("loop back through channel IQ:", sum(k["loopback"] for k in ks), "cases")
    assert sum(k["loopback"] for k in ks) >= 10
    for k in ks:
        assert len(k["calls"]) == 6 and k["calls"][0] == max(k["calls"]) and 2 <= k["edit_call"] <= 5
        assert sum(c < k["calls"][0] for c in k["calls"]) >= 3
        q = 8 * k["D"] if k["cic"] else 1  # the short call: the smallest the geometry takes (the CIC rule kept)
        assert fc.min_samples(k, oracle) <= k["calls"][2] < fc.min_samples(k, oracle) + q
        assert k["shared"] or k["edit"] != "switch"
        assert not k["shared"] or k["table"] >= 1
        if k["cic"]:
            assert all(c % (8 * k["D"]) == 0 for c in k["calls"])


def test_feed_taps_fit_at_every_rate(oracle):
    """between 2 and 75 taps (the kernel's cap) for both divisors at the three PCM rates"""
    for pcm in fc.PCM:
        for dv in (2, 3):
            t = fc.feed_taps(dict(pcm=pcm, feed_div=dv), oracle)
            print("pcm %g / %d: %d taps" % (pcm, dv, t.size))
            assert 2 <= t.size <= 75


def test_streams_hold_what_the_gpu_test_needs(oracle, fmsig):
    s16_frames, m_mod4, m_mod64, p0, parity = set(), set(), set(), set(), set()
    clip_cases = feed_sat = mpx_sat = group_cases = 0
    status, offsets = set(), set()
    for k, e in _all(oracle, fmsig):
        any_clip = any_feed = any_mpx = any_group = False
        for c, ch in e["ch"].items():
            for j, call in enumerate(ch["calls"]):
                w = k["outs"][j]
                if w["audio"] == "s16":
                    s16_frames.add(call["frames"] % 4)
                if w["mpx"] or w["ciq"]:
                    m_mod4.add(call["M"] % 4)
                    m_mod64.add(call["M"] % 64)
                if w["feed"]:
                    p0.add((k["feed_div"], call["g0"] % k["feed_div"]))
                    parity.add(call["feed"].size % 2)
                    if w["feed"] == "s16":
                        any_feed |= bool(fc.clipped(call["feed_f32"]).any())
                if w["mpx"] == "s16":
                    any_mpx |= bool((np.abs(call["mpx"].astype(np.int32)) >= 32767).any())
            any_clip |= ch["clip"] > 0
            any_group |= len(ch["groups"]) > 0
            status |= set(ch["records"]["status"].tolist())
            offsets |= set(ch["records"]["position"].tolist())
            # rds_sync_spec at this geometry: its groups are the oracle's, call by call
            assert [(a, tuple(b)) for a, b in ch["spec_groups"]] == [(a, tuple(b)) for a, b in ch["groups"]], \
                (k["seed"], c)
        clip_cases += any_clip
        feed_sat += any_feed
        mpx_sat += any_mpx
        group_cases += any_group
    print("S16 frames mod 4", sorted(s16_frames), "M mod 4", sorted(m_mod4), "M mod 64 edge",
          sorted(m_mod64 & {0, 1, 63}), "feed phases", sorted(p0), "feed count parities", sorted(parity))
    print("cases with: clip count", clip_cases, "saturated S16 feed", feed_sat, "saturated S16 MPX", mpx_sat,
          "groups", group_cases, "| record statuses", sorted(status), "offset words", sorted(offsets))
    assert status == {0, 1, 2} and len(offsets) >= 4 and group_cases >= fc.N_DEFAULT // 2
    assert s16_frames == {0, 1, 2, 3} and m_mod4 == {0, 1, 2, 3} and m_mod64 >= {0, 1, 63}
    assert p0 == {(2, 0), (2, 1), (3, 0), (3, 1), (3, 2)} and parity == {0, 1}
    assert clip_cases >= 4 and feed_sat >= 3 and mpx_sat >= 3
