"""The scripts of tests/edit_model.py have bite: shown on the CPU oracle alone, no GPU.

What tests/test_gpu_edits_ragged.py compares a batch with is only worth something if the scripts reach the places the
edit code can be wrong in: resets at non-zero ring phases, followed by calls with fewer RDS rows than the ring filters
have taps; RDS groups on both sides of the edits; retunes whose zero history depends on the call sizes."""
import pytest

import edit_model as em
from test_gpu_reset_channels import SHIFTS0

LOUD_PI = 0x7011


def build(oracle, fmsig, name):
    """(script, model) of a named script, as tests/test_gpu_edits_ragged.py runs it"""
    script, _, model, _, _ = em.build(oracle, fmsig, name)
    return script, model


ALL = ["resets", "retunes", "switches", "state", "flight", "shell8"] + ["random%d" % s for s in em.RANDOM_SEEDS]


@pytest.mark.parametrize("name", ALL)
def test_resets_are_at_non_zero_ring_phases(oracle, fmsig, name):
    """At every per-channel reset of every script both ring phases of the batch are non-zero: the reset channel's
    origin differs from the batch's phase in the low-pass and in the matched filter."""
    _, m = build(oracle, fmsig, name)
    o = em._oracle(oracle, 0)
    assert (len(o.rds_lpf_taps()), len(o.rds_mf_taps())) == (em.T_LPF, em.T_MF)
    report = m.reset_report()
    print(name, "decoders", m.decoders, "rows", m.R)
    for k, b, ch, ph, rows in report:
        print("  reset in front of call %d, batch %d, channels %s: phases %s, rows from there %s"
              % (k, b, ch, ph, rows))
        assert ph[0] != 0 and ph[1] != 0, (name, k, ph)
    if name != "switches":
        assert report, name


@pytest.mark.parametrize("name", ["resets", "retunes", "flight", "shell8"] + ["random%d" % s for s in em.RANDOM_SEEDS])
def test_a_reset_is_followed_by_a_run_of_short_rows(oracle, fmsig, name):
    """At least one reset is followed by four or more consecutive calls with fewer RDS rows than the matched filter
    has taps (R < 44), one of them with R = 1: the reset channel's rings wrap across calls while k_roll moves fewer
    rows than the history holds."""
    _, m = build(oracle, fmsig, name)
    best = 0
    for k, _, _, _, rows in m.reset_report(follow=12):
        run = 0
        while run < len(rows) and rows[run] < em.T_MF:
            run += 1
        if 1 in rows[:run]:
            best = max(best, run)
    assert best >= 4, (name, best)


@pytest.mark.parametrize("seed", em.RANDOM_SEEDS)
def test_random_scripts_hold_every_edit_kind(oracle, fmsig, seed):
    _, m = build(oracle, fmsig, "random%d" % seed)
    kinds = {kind for _, _, kind, _ in m.events}
    assert kinds == set(em.KINDS), kinds
    assert len(m.script) >= 40


def _loud_groups(m, k0, k1):
    """groups of the loud station (its PI code in block A) that any slot of any batch delivers in calls [k0, k1)"""
    seen = set()
    n = 0
    for k in range(k0, k1):
        for b in range(len(m.C)):
            for node in set(m.at_[k][b]):
                if (k, node) not in seen:
                    seen.add((k, node))
                    n += sum(1 for blk in m.rec[node]["groups"] if blk[0] == LOUD_PI)
    return n


@pytest.mark.parametrize("name", ["resets", "retunes", "switches", "state", "flight"]
                         + ["random%d" % s for s in em.RANDOM_SEEDS])
def test_loud_station_delivers_groups_on_both_sides_of_every_edit(oracle, fmsig, name):
    """Counting every decoder lineage once: the loud station's groups arrive before and behind every boundary with an
    edit -- at least 1 before (the first edits come behind 7 or 8 full calls: the first group is the 7th call's) and
    at least 2 behind (8 or 9 full calls end every script) in every script, on the oracle alone -- and at least one
    decoder that an edit made or changed delivers them behind its edit."""
    script, m = build(oracle, fmsig, name)
    worst = [10 ** 9, 10 ** 9]
    for k in sorted({k for k, _, _, _ in m.events}):
        before, behind = _loud_groups(m, 0, k), _loud_groups(m, k, len(script))
        worst = [min(worst[0], before), min(worst[1], behind)]
    print(name, "fewest groups before / behind an edit:", worst)
    assert worst[0] >= 1 and worst[1] >= 2, (name, worst)
    edited = 0
    for k, b, kind, ch in m.events:
        if kind in ("reset", "retune", "retune_to", "switch", "move"):
            for c in ch:
                edited += sum(1 for j in range(k, len(script)) for blk in m.at(j, c, b)["groups"] if blk[0] == LOUD_PI)
    print(name, "groups of edited decoders behind their edits:", edited)
    assert edited >= 1, name


def test_the_sizes_of_the_earlier_calls_matter(oracle, fmsig):
    """A retuned decoder whose earlier calls were zeros of 65 536 samples each, not of the real sizes, gives other
    bits: slots 5 and 6 of "retunes" (retuned in front of call 11, behind calls of 88, 150 and 300 samples) differ from
    the right model in the audio of that very call, slot 6 (the loud station) also in its matched filter's rows of the
    next; slots 3 and 4 (retuned behind eight full calls: both histories are the same) do not differ."""
    script, right = build(oracle, fmsig, "retunes")
    wrong = em.Model(oracle, right.streams, script, SHIFTS0, [0] * 8, wrong_history=65536)
    assert [(k, kind, ch) for k, _, kind, ch in right.events[:3]] == \
        [(8, "retune", [3, 4]), (11, "retune_to", [5, 6]), (13, "reset", [2, 6])]
    for c in (5, 6):
        assert not em._bits(right.at(11, c)["audio"], wrong.at(11, c)["audio"]), c
    for c in (3, 4):
        for k in range(8, 11):
            assert em._bits(right.at(k, c)["audio"], wrong.at(k, c)["audio"]), (c, k)
    assert not em._bits(right.at(12, 6)["taps"]["rds_mf"], wrong.at(12, 6)["taps"]["rds_mf"])
