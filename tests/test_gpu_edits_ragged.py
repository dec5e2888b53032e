"""Per-channel edits of a running batch at ragged call sizes, bit for bit.

reset_channels, retune (with and without a capture), switch_captures, export / import and save / load happen at call
boundaries, and what they copy, zero or re-base is state whose shape depends on the sizes of the calls around the
boundary.  Here the edits meet calls of 88 .. 40 000 samples mixed with full ones: every comparison is an equality
against the oracle model of tests/edit_model.py (one decoder lineage per history, following include/fmd.h) or against
another run of the same script.  tests/test_edit_model_cpu.py shows on the oracle alone that the scripts reach what
they are meant to: the ring phases at every reset, the runs of calls with fewer RDS rows than the ring filters have
taps, the groups on both sides of the edits.

Geometry: 2.4 MS/s, D = 11, min_samples() == 88 (the long-filter cases apart)."""
import numpy as np
import pytest

import edit_model as em
from __graft_entry__ import load_package
from test_gpu_reset_channels import SHIFTS0, _bits
from test_gpu_state import FMD_ERR_STATE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def _status_words(s):
    return (int(s.stereo_detected), int(s.rds_state), np.array([s.tuning_offset, s.interface_level, s.baseband_level,
                                                                s.pilot_level], np.float32).tobytes())


# ---------------------------------------------------------------------------------------------------------------------
# resets

@pytest.mark.parametrize("ring4,u8,mode", [(1, False, "device"), (0, False, "device"), (1, True, "host"),
                                           (0, True, "device")],
                         ids=["ring4-f32", "lds-f32", "ring4-u8-host", "lds-u8"])
def test_resets(pkg, oracle, fmsig, ring4, u8, mode):
    """Script "resets": 8 channels (one wave of mixed origins) on one shared capture.  Channels 0 and 5 are reset in
    front of a call of 88 samples (ring phases 35 / 20), followed by calls of 88, 97, 150, 300, 170 and 89 samples
    (R = 1, 1, 1, 1, 3, 2, 1: the matched filter's ring of a reset channel wraps across calls); 1 and 0 (again) behind
    that run, in front of 100 samples (R = 1, then 42, 3, 11); 2 in front of 8191; the whole batch is reset, and 0
    and 3 are reset two calls behind that (phases 72 / 43).  Every channel follows the model in the audio, the getters
    and the three RDS taps of every call, the RDS groups (device calls) and UECP frames of every call, and the PS name;
    with the ring filters' register form (ring4 = 1) and their LDS form (0), float and byte input."""
    script, streams, m, shifts, _ = em.build(oracle, fmsig, "resets", u8)
    drv = em.Driver(pkg, streams, shifts, mode=mode, enable=False, debug={"ring4": ring4}, taps_of=range(8))
    assert drv.units[0].b.min_samples() == 88
    res = drv.play(script)
    drv.finish()
    em.check_model(m, drv, res)
    em.check_names(m, drv)
    assert sum(len(m.at(k, 0)["frames"]) for k in range(25, len(script))) > 0  # behind the last reset of channel 0


def test_resets_keep_phase_has_teeth(pkg, oracle, fmsig):
    """With fmd_batch_debug_reset_keep_ring_phase the reset channels keep the batch's ring phase: everything before
    the first reset (call 8) still agrees, and the low-pass and matched-filter taps of channels 0 and 5 then differ
    from the model's somewhere in the seven calls behind it (not in the first: one row over an empty history is one
    product whatever the ring's phase), those of channel 3 behind its reset at call 25; a channel that was not reset
    does not differ."""
    script, streams, m, shifts, _ = em.build(oracle, fmsig, "resets")
    drv = em.Driver(pkg, streams, shifts, mode="device", enable=False, taps_of=range(8), keep_phase=True)
    res = drv.play(script)
    drv.finish()
    em.check_model(m, drv, res, calls=range(8))
    for c, calls in ((0, range(8, 15)), (5, range(8, 15)), (3, range(25, 29))):
        for t in ("rds_lpf", "rds_mf"):
            differs = [k for k in calls if em.taps_differ(m, res, k, c)[t]]
            print("channel %d, %s differs in calls %s" % (c, t, differs))
            assert differs, (c, t)
    em.check_model(m, drv, res, channels=[4, 6, 7], calls=range(8, 22))


# ---------------------------------------------------------------------------------------------------------------------
# retunes

@pytest.mark.parametrize("u8,mode", [(False, "device"), (True, "host")], ids=["f32", "u8-host"])
def test_retunes(pkg, oracle, fmsig, u8, mode):
    """Script "retunes": 8 channels over two capture rows, retuning enabled.  Retunes in front of a call of 88 samples
    behind eight full ones; to a capture behind calls of 88, 150 and 300 (the silent twin's regions are partly refilled
    there, not filtered); of slot 2 in front of 3663 samples, one call behind its reset in front of 97; behind 330 and
    100; in front of 1001.  Every channel follows the model (a decoder of the new shift that received zeros of the
    real sizes) in everything test_resets compares."""
    script, streams, m, shifts, cmaps = em.build(oracle, fmsig, "retunes", u8)
    drv = em.Driver(pkg, streams, shifts, cmaps, mode=mode, taps_of=range(8))
    res = drv.play(script)
    drv.finish()
    em.check_model(m, drv, res)
    em.check_names(m, drv)
    assert sum(len(m.at(k, 7)["frames"]) for k in range(22, len(script))) > 0  # slot 7: the loud station at the end


# ---------------------------------------------------------------------------------------------------------------------
# capture switches

def test_switches(pkg, oracle, fmsig):
    """Script "switches" on the 88-tap geometry: switches in front of calls of 89, 300, 100, 8191 and 40 000 samples,
    there and back within three tiny calls.  The demod tap (the IF filter's window holds both captures), the RDS taps,
    audio, getters, groups and frames of every channel in every call."""
    script, streams, m, shifts, cmaps = em.build(oracle, fmsig, "switches")
    drv = em.Driver(pkg, streams, shifts, cmaps, mode="device", enable=False, taps_of=range(8),
                    tap_names=em.RDS_TAPS + ("demod",))
    res = drv.play(script)
    drv.finish()
    em.check_model(m, drv, res)
    em.check_names(m, drv)


@pytest.mark.parametrize("fs,d", [(2.4e6, 11), (1.4e6, 6)])
def test_switches_and_a_save_inside_a_long_filter(pkg, oracle, fmsig, fs, d):
    """IF filters of order 1000 (D = 11, and D = 6: the two-region window of test_long_filters_and_even_decimation):
    switches in front of calls of 500, 900 and 333 samples splice two captures inside one filter window, and the batch
    is saved behind a call of 700 samples (shorter than the filter), destroyed and loaded.  The demod tap, audio and
    getters of every call against the oracle on the spliced stream."""
    geom = em.Geometry(fs, d, em.T, 1000)
    script = em.SCRIPTS["long"]
    streams = em.long_streams(fmsig, geom, em.total_samples(script))
    m = em.Model(oracle, streams, script, em.SHIFTS_LONG, em.CMAP_LONG, geom=geom, taps=("demod",))
    drv = em.Driver(pkg, streams, em.SHIFTS_LONG, em.CMAP_LONG, mode="device", geom=geom, enable=False,
                    taps_of=range(4), tap_names=("demod",))
    assert min(n for n, _ in script) >= drv.units[0].b.min_samples()
    res = drv.play(script)
    drv.finish()
    em.check_model(m, drv, res)


# ---------------------------------------------------------------------------------------------------------------------
# state

def test_state(pkg, oracle, fmsig):
    """Script "state": batches A and B over two capture rows, fed the same ragged sizes.  Both are saved directly
    behind an R = 1 call (88 samples), destroyed and loaded into fresh batches that continue ragged; A's channels 0, 1
    and 5 move into B's slots 6, 2 and 3 behind calls of 97 and 3663 samples, in front of one of 150; B is saved and
    loaded again behind 89 samples with the moved decoders in it, and a moved slot is reset after that.  Every channel
    of both batches follows the model in everything test_resets compares."""
    script, streams, m, shifts, cmaps = em.build(oracle, fmsig, "state")
    drv = em.Driver(pkg, streams, shifts, cmaps, mode="device", taps_of=range(8))
    res = drv.play(script)
    drv.finish()
    for b in (0, 1):
        em.check_model(m, drv, res, b=b)
        em.check_names(m, drv, b=b)
    assert sum(len(m.at(k, 6, 1)["groups"]) for k in range(12, 24)) > 0  # the loud station in B's slot 6


def test_clock_rule_one_tiny_call_apart(pkg, oracle, fmsig):
    """B has had one call of 88 samples more than A (65 536, 300, 97 against 65 536, 300, 88, 97): the import is
    refused with FMD_ERR_STATE naming the first differing word, nothing is queued, and B carries on exactly."""
    script_a = em._steps(em.F, 300, 97)
    script_b = em._steps(em.F, 300, 88, 97, 150, em.F)
    streams = em.main_streams(fmsig, em.total_samples(script_b))
    a = em.Driver(pkg, streams, SHIFTS0, mode="device")
    a.play(script_a)
    blob = a.units[0].b.export_channels([0, 1, 5])
    a.finish()
    m = em.Model(oracle, streams, script_b, em.SHIFTS_B)
    b = em.Driver(pkg, streams, em.SHIFTS_B, mode="device", taps_of=range(8))
    b.play(script_b, upto=4)
    with pytest.raises(pkg.FmdError, match=FMD_ERR_STATE) as e:
        b.units[0].b.import_channels([6, 2, 3], blob)
    print(str(e.value))
    assert "first in" in str(e.value), str(e.value)
    words = ("if_pos", "lut_idx", "rs_pos", "rds_lpf_g", "mf_g", "alpf_g", "hist_sel", "call_index", "osc_")
    assert any(w in str(e.value) for w in words), str(e.value)
    res = b.play(script_b)
    b.finish()
    em.check_model(m, b, res)


# ---------------------------------------------------------------------------------------------------------------------
# calls in flight

@pytest.fixture(scope="module")
def flight_serial(pkg, oracle, fmsig):
    """script "flight" one call at a time: every channel of both batches against the model, and what the runs with
    calls in flight are compared with"""
    script, streams, m, shifts, cmaps = em.build(oracle, fmsig, "flight")
    drv = em.Driver(pkg, streams, shifts, cmaps, mode="device", status_of=[])
    res = drv.play(script)
    last = drv.finish()
    for b in (0, 1):
        em.check_model(m, drv, res, b=b, what=("audio", "groups", "frames"))
        em.check_names(m, drv, b=b)
    return drv, res, last


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("lag", [1, 2, 3])
def test_edits_with_calls_in_flight(pkg, oracle, fmsig, flight_serial, lag, layout):
    """Script "flight": two batches of 130 channels (three waves, the last partial) over two captures at concurrency
    2, the outputs consumed `lag` calls late, in each stream layout of an overlapped call ("lpf_late").  Resets,
    retunes (to a capture too), switches, a save / load, a move between the batches and a whole-batch reset are made
    while earlier calls still run; the host works out every one of them from the call sizes alone.  Every channel's
    audio of every call, its groups with their call index, UECP frames, PS names and the getters behind the last call
    equal the run of one call at a time; one channel per decoder lineage is compared with the model directly."""
    script, streams, m, shifts, cmaps = em.build(oracle, fmsig, "flight")
    serial, want, last_want = flight_serial
    drv = em.Driver(pkg, streams, shifts, cmaps, mode="flight", lag=lag, debug={"lpf_late": layout}, status_of=[])
    res = drv.play(script)
    drv.status_of = None
    last = drv.finish()
    for b in (0, 1):
        for k in range(len(script)):
            got, ref = res[k][b]["audio"], want[k][b]["audio"]
            assert got.shape == ref.shape, (k, b)
            bad = np.flatnonzero((got.view(np.uint32) != ref.view(np.uint32)).any(axis=1))
            assert bad.size == 0, ("audio", k, script[k][0], b, bad[:8])
        assert sorted(drv.groups[b]) == sorted(g for k in range(len(script)) for g in want[k][b]["groups"]), b
        assert drv.frames[b] == serial.frames[b], b
        assert len(drv.groups[b]) > 100 and len(drv.frames[b]) > 30, (b, len(drv.groups[b]), len(drv.frames[b]))
        assert drv.names[b] == serial.names[b], b
        for c in m.one_per_lineage(b):
            for k in range(len(script)):
                assert _bits(res[k][b]["audio"][c], m.at(k, c, b)["audio"]), (k, b, c)
        for c in range(130):
            s, ci = last[b][c]
            assert em._status_equal(s, m.at(len(script) - 1, c, b)["status"]), (b, c)
            assert ci == len(script), (b, c)


# ---------------------------------------------------------------------------------------------------------------------
# sub-batches

def test_edits_across_sub_batches(pkg, oracle, fmsig):
    """Script "shell8" on a shell of 16 384 channels (two sub-batches) on one shared capture row, calls of at most
    8192 samples, every edit made on whole residue classes mod 8 (2048 channels on both sides of the border, one in
    every eight lanes of every wave: mixed origins everywhere): channel c equals channel c % 8 of an 8-channel batch run
    through the same script -- audio and groups of every call, the getters of channels around the border -- and that
    batch follows the model."""
    script, streams, m, shifts, _ = em.build(oracle, fmsig, "shell8")
    small = em.Driver(pkg, streams, shifts, mode="device", taps_of=range(8))
    want = small.play(script)
    small.finish()
    em.check_model(m, small, want)
    C_ = 16384
    look = [0, 5, 8189, 8191, 8192, 8197, 16379, 16383]
    shell = em.Driver(pkg, streams, [int(x) for x in np.resize(np.array(shifts, np.int32), C_)], mode="device",
                      status_of=look, callbacks=False)
    res = shell.play(em.widen(script, 8, C_))
    shell.finish()
    cls = np.arange(C_) % 8
    for k in range(len(script)):
        got, ref = res[k][0]["audio"], want[k][0]["audio"][cls]
        assert got.shape == ref.shape and got.shape[0] == C_ and np.any(got[8192:]), k
        bad = np.flatnonzero((got.view(np.uint32) != ref.view(np.uint32)).any(axis=1))
        assert bad.size == 0, ("audio", k, script[k][0], bad[:8])
        assert sorted((c % 8, ci, blk) for c, ci, blk in res[k][0]["groups"]) == \
            sorted((c, ci, blk) for c, ci, blk in want[k][0]["groups"] for _ in range(C_ // 8)), k
        for c in look:
            assert _status_words(res[k][0]["status"][c][0]) == _status_words(want[k][0]["status"][c % 8][0]), (k, c)
            assert res[k][0]["status"][c][1] == k + 1, (k, c)


# ---------------------------------------------------------------------------------------------------------------------
# random walks

@pytest.mark.parametrize("seed", em.RANDOM_SEEDS)
def test_random_walk(pkg, oracle, fmsig, seed):
    """em.random_script(seed): 41 calls on two batches of 8 channels over two captures, the sizes drawn from the edge
    set and from random values, the edits from the whole vocabulary (tests/test_edit_model_cpu.py asserts what the
    scripts hold).  Every channel of both batches follows the model in everything test_resets compares."""
    script, streams, m, shifts, cmaps = em.build(oracle, fmsig, "random%d" % seed)
    assert {kind for _, _, kind, _ in m.events} == set(em.KINDS)
    for k, b, ch, ph, rows in m.reset_report():
        assert ph[0] != 0 and ph[1] != 0, (k, ph)
    drv = em.Driver(pkg, streams, shifts, cmaps, mode="device", taps_of=range(8))
    res = drv.play(script)
    drv.finish()
    for b in (0, 1):
        em.check_model(m, drv, res, b=b)
        em.check_names(m, drv, b=b)
