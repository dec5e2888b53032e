"""The restated slicer and block machine (tests/rds_sync_spec.py) IS the reference's: on every stream the GPU tests of
the block observation use, its groups are the oracle's, with the oracle's 1-based call index.  And the streams are
worth testing on: together they hold every kind of record there is, several times, and version-B groups (offset word
C').  Without this the GPU tests could pass on nothing."""
import numpy as np

import rds_blocks_cases as cases
import rds_sync_spec as spec


def _streams(oracle, fmsig):
    out = {}
    for cap, shift in cases.MIXED_STREAMS:
        out[("mixed", cap, shift)] = cases.mixed_spec(oracle, fmsig, cap, shift)
    out[("ragged",)] = cases.oracle_spec(oracle, cases.plain_020(fmsig), cases.SHIFT_A, "ragged")
    out[("ragged", "reset")] = cases.oracle_spec(oracle, cases.plain_020(fmsig), cases.SHIFT_A, "ragged", resets=(30,))
    out[("ragged", "u8")] = cases.oracle_spec(oracle, cases.plain_020(fmsig, u8=True), cases.SHIFT_A, "ragged-u8",
                                               u8=True)
    return out


def test_check_block_knows_the_offset_words(fmsig):
    # the generator's own blocks (a version-A and a version-B group): each passes against its own offset word only
    groups = [(0x7011, 0x0408, 0xE0CD, 0x4C4F), (0x7011, 0x0C08, 0x7011, 0x4C4F)]
    d = fmsig.sched_dbits(groups).astype(np.int64)
    bits = d ^ np.concatenate([d[-1:], d[:-1]])  # differential decoding; the table loops
    blocks = [int("".join(map(str, bits[26 * j:26 * j + 26])), 2) for j in range(8)]
    want = [0, 1, 2, 3, 0, 1, 6, 3]  # entries of OFFSETS: the second group's third block carries C'
    for j, block in enumerate(blocks[1:], 1):  # (the first block's first bit depends on the loop's last: skip it)
        assert block >> 10 == groups[j // 4][j % 4]
        for idx, off in enumerate(spec.OFFSETS):
            _, syn, pre, flips = spec.check_block(block, off, False)
            assert (syn == 0) == (off == spec.OFFSETS[want[j]]) and pre == syn and flips == 0, (j, idx)
    # one flipped bit: fails without the error correction, is repaired with it and counted
    block, off = blocks[1], spec.OFFSETS[1]
    assert spec.check_block(block ^ (1 << 20), off, False)[1] != 0
    after, syn, pre, flips = spec.check_block(block ^ (1 << 20), off, True)
    assert (after & 0x3FFFFFF, syn, flips) == (block, 0, 1) and pre != 0


def test_the_specs_groups_are_the_oracles(oracle, fmsig):
    for key, (s, _audio, groups) in _streams(oracle, fmsig).items():
        assert s.groups == groups, (key, len(s.groups), len(groups))
        q = dict(zip(spec.QUALITY_FIELDS, s.quality()))
        r = s.records_array()
        assert q["groups"] == len(groups) and q["blocks"] + q["candidates"] == len(r), key


def test_the_streams_hold_every_kind_of_record(oracle, fmsig):
    total, pos4, version_b = {}, 0, 0
    for key, (s, _audio, groups) in _streams(oracle, fmsig).items():
        r = s.records_array()
        for k, n in cases.kinds(r).items():
            total[k] = total.get(k, 0) + n
        pos4 += int((r["position"] == 4).sum())
        version_b += sum(1 for _ci, g in groups if g[1] & 0x0800)
    print(sorted(total.items()), pos4, version_b)
    for k in [(0, 0), (1, 0), (1, 2), (2, 0), (2, 1), (2, 2)]:
        assert total.get(k, 0) >= 3, (k, total)
    assert set(total) <= {(0, 0), (1, 0), (1, 2), (2, 0), (2, 1), (2, 2)}, total
    assert version_b >= 1 and pos4 >= 1


def test_a_machine_reset_keeps_the_counters():
    s = spec.SyncSpec()
    s.q["bits"] = 77
    s.m.state, s.m.in_bits = spec.GROUPDECODE, 0x1234
    s.reset_machine()
    assert s.m.state == spec.BITSYNC and s.m.in_bits == 0x1234 and s.quality()[0] == 77
