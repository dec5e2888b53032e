"""Every RDS block decision and the per-channel reception counters (fmd_batch_set_rds_blocks and its kin, include/fmd.h,
DESIGN.md section 9.10).

No tolerance anywhere: every value is an integer the reference's own state machine computes.  Expected values are the
restated machine of tests/rds_sync_spec.py on the CPU oracle's taps (shown to be the oracle's machine by
tests/test_rds_sync_spec.py); beyond the oracle's reach every record is checked against a Python CheckBlock of its own
raw / position / state and against the groups the batch delivers.  Every comparison is an equality."""
import numpy as np
import pytest

import rds_blocks_cases as cases
import rds_sync_spec as spec
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
FS, D, TABLE, N = cases.FS, cases.D, cases.TABLE, cases.N


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def _params(pkg):
    return pkg.make_params(FS, 0.0, 48000.0, 15000.0, D, table_size=TABLE)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _sorted(recs):
    """the order fmd_batch_collect_rds_blocks promises: (call_index, channel, bit_index)"""
    key = list(zip(recs["call_index"].tolist(), recs["channel"].tolist(), recs["bit_index"].tolist()))
    return key == sorted(key)


def _same_records(recs, quality, want):
    """recs / quality of a batch against {channel: SyncSpec}: all ten fields of every record, all eight counters"""
    assert recs.dtype == spec.BLOCK_DTYPE
    assert set(np.unique(recs["channel"]).tolist()) <= set(want)
    for c, s in want.items():
        got = recs[recs["channel"] == c]
        exp = s.records_array().copy()
        exp["channel"] = c
        assert len(got) == len(exp), (c, len(got), len(exp))
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, (c, bad.size, got[bad[:3]], exp[bad[:3]])
        assert tuple(int(x) for x in quality[c]) == s.quality(), (c, quality[c], s.quality())


def _status_tuple(b, c):
    s = b.status(c)
    vals = (s.tuning_offset, s.interface_level, s.baseband_level, s.pilot_level) + tuple(b.audio_level(c))
    return (s.stereo_detected, s.rds_state) + tuple(int(np.float32(v).view(np.uint32)) for v in vals)


# ---- 1. mixed lanes -------------------------------------------------------------------------------------------------
def test_mixed_lanes_equal_the_spec_and_leave_the_decoder_alone(pkg, oracle, fmsig):
    Cn = 130
    caps = cases.captures(fmsig, "mixed")
    stream_of = [c % len(cases.MIXED_STREAMS) for c in range(Cn)]  # neighbouring lanes read different captures
    cmap = np.array([cases.MIXED_STREAMS[s][0] for s in stream_of], np.uint32)
    shifts = np.array([cases.MIXED_STREAMS[s][1] for s in stream_of], np.int32)
    b = pkg.Batch(_params(pkg), Cn, tuning_shifts=shifts)
    b0 = pkg.Batch(_params(pkg), Cn, tuning_shifts=shifts)  # never enables the mode
    for x in (b, b0):
        x.set_capture_map(cmap, cases.N_CAPTURES)
    assert b.rds_blocks() == 0
    b.set_rds_blocks(pkg.FMD_RDS_BLOCKS_RECORD)
    assert b.rds_blocks() == 2 and b0.rds_blocks() == 0
    got, lost_all = [], 0
    for k, x in enumerate(caps):
        a, a0 = b.process_host_fmt(x), b0.process_host_fmt(x)
        assert a.shape == a0.shape and (_bits(a) == _bits(a0)).all(), k
        if k % 8 == 7:
            r, lost = b.collect_rds_blocks(cap=1 << 16)
            assert _sorted(r)
            got.append(r)
            lost_all += lost
    r, lost = b.collect_rds_blocks(cap=1 << 16)
    got.append(r)
    recs = np.concatenate(got)
    assert lost_all + lost == 0 and _sorted(recs)
    want = {}
    for c in range(Cn):
        cap, shift = cases.MIXED_STREAMS[stream_of[c]]
        want[c] = cases.mixed_spec(oracle, fmsig, cap, shift)[0]
    _same_records(recs, b.rds_quality(), want)
    assert not b0.rds_quality().view(np.uint32).any()  # a batch that never enabled it: zeros, nothing allocated
    assert cases.kinds(recs).keys() >= {(0, 0), (1, 0), (1, 2), (2, 0), (2, 1), (2, 2)} and (recs["position"] == 4).any()
    # audio (above), groups -- the host call feeds them to the group decoders -- and status bits
    assert b.sink.frames == b0.sink.frames and b.sink.names == b0.sink.names and len(b.sink.frames) > 0
    assert [_status_tuple(b, c) for c in range(Cn)] == [_status_tuple(b0, c) for c in range(Cn)]
    r, lost = b0.collect_rds_blocks(cap=16)
    assert len(r) == 0 and lost == 0
    b.close()
    b0.close()


# ---- 2. edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn,u8", [(1, False), (63, False), (65, False), (65, True)])
def test_ragged_calls_and_partial_waves(pkg, oracle, fmsig, Cn, u8):
    blocks = cases.plain_020(fmsig, u8=u8)
    want, _audio, groups = cases.oracle_spec(oracle, blocks, cases.SHIFT_A, "ragged-u8" if u8 else "ragged", u8=u8,
                                             resets=() if u8 else (30,))
    b = pkg.Batch(_params(pkg), Cn, tuning_shifts=np.full(Cn, cases.SHIFT_A, np.int32), record_callbacks=False)
    assert b.min_samples() <= min(cases.RAGGED)
    b.set_rds_blocks(2)
    got = []
    for k, x in enumerate(blocks):
        if k == 30 and not u8:
            b.reset()  # restarts the machine where it always did; the counters run on
        b.process_host_fmt(x, shared=True)
        if k % 7 == 6:
            got.append(b.collect_rds_blocks()[0])
    got.append(b.collect_rds_blocks()[0])
    recs = np.concatenate(got)
    assert _sorted(recs) and int(recs["sample"].max()) > 32  # (rows longer than one tile)
    _same_records(recs, b.rds_quality(), {c: want for c in range(Cn)})
    assert tuple(b.rds_quality(Cn - 1, 1)[0].tolist()) == want.quality()
    b.close()


# ---- 3. in flight ---------------------------------------------------------------------------------------------------
_MODES = [0, 1, 2, 2, 1, 0, 2, 0, 1, 2, 1, 2] * 2
_FLIGHT_SHIFTS = (cases.SHIFT_A, cases.SHIFT_B, cases.SHIFT_EMPTY)


def _flight(pkg, fmsig, conc, lag, setup):
    """24 calls of capture 2 (one shared row) on 65 channels, the mode changed in front of every call, submitted back
    to back; records and groups collected lagged, each at its own cadence"""
    import torch
    Cn = 65
    caps = cases.captures(fmsig, "mixed")[:len(_MODES)]
    shifts = np.array([_FLIGHT_SHIFTS[c % 3] for c in range(Cn)], np.int32)
    b = pkg.Batch(_params(pkg), Cn, tuning_shifts=shifts, record_callbacks=False)
    b.set_concurrency(conc)
    if setup:
        b.debug_set(*setup)
    st = torch.cuda.current_stream().cuda_stream
    a_stride = (b.max_audio_floats(N) + 7) // 8 * 8
    keep, audio, nfs, recs, groups, quality = [], [], [], [], [], []
    for k, x in enumerate(caps):
        d_iq = torch.from_numpy(np.ascontiguousarray(x[2])).cuda()
        out = torch.zeros((Cn, a_stride), dtype=torch.float32, device="cuda")
        keep.append(d_iq)
        audio.append(out)
        b.set_rds_blocks(_MODES[k])
        nfs.append(b.process_device(d_iq.data_ptr(), 0, N, out.data_ptr(), a_stride, st))
        if conc == 2 and k >= lag:
            r, lost = b.collect_rds_blocks(lag=lag, stream=st)
            assert lost == 0 and (len(r) == 0 or int(r["call_index"].max()) <= k + 1 - lag)
            recs.append(r)
            if k % 3 == 0:
                groups.append(b.collect_rds_array(stream=st, lag=lag))
        if k == 11:
            quality.append(b.rds_quality())  # synchronous: every call submitted so far
    b.wait(stream=st)
    torch.cuda.synchronize()
    r, lost = b.collect_rds_blocks(stream=st)
    assert lost == 0
    recs.append(r)
    groups.append(b.collect_rds_array(stream=st))
    quality.append(b.rds_quality())
    res = {"recs": np.concatenate(recs), "groups": np.sort(np.concatenate(groups), order=["channel", "call_index"]),
           "audio": [a.cpu().numpy()[:, :nf] for a, nf in zip(audio, nfs)], "quality": quality}
    b.close()
    return res


@pytest.fixture(scope="module")
def serial_flight(pkg, fmsig):
    return _flight(pkg, fmsig, 0, 0, None)


def test_the_serial_flight_equals_the_spec(pkg, oracle, fmsig, serial_flight):
    blocks = [x[2] for x in cases.captures(fmsig, "mixed")[:len(_MODES)]]
    s = [cases.oracle_spec(oracle, blocks, sh, ("flight", 2), modes=_MODES)[0] for sh in _FLIGHT_SHIFTS]
    half = [cases.oracle_spec(oracle, blocks[:12], sh, ("flight12", 2), modes=_MODES[:12])[0] for sh in _FLIGHT_SHIFTS]
    r = serial_flight
    _same_records(r["recs"], r["quality"][-1], {c: s[c % 3] for c in range(65)})
    for c in range(65):  # counters move only in calls of mode >= 1
        assert tuple(int(x) for x in r["quality"][0][c]) == half[c % 3].quality()
    mode2 = {k + 1 for k, m in enumerate(_MODES) if m == 2}
    assert set(np.unique(r["recs"]["call_index"]).tolist()) <= mode2 and len(r["recs"]) > 0
    assert sum(len(x.groups) for x in s) > 0
    for c in range(3):  # the groups are the machine's whatever the mode
        g = r["groups"][r["groups"]["channel"] == c]
        assert [(int(k), tuple(int(v) for v in bl)) for k, bl in zip(g["call_index"], g["blocks"])] == s[c].groups


@pytest.mark.parametrize("lag", [1, 2, 3])
@pytest.mark.parametrize("how", ["default", "split_post", "lpf_late0", "lpf_late1", "lpf_late2"])
def test_modes_of_calls_in_flight(pkg, fmsig, serial_flight, how, lag):
    setup = {"default": None, "split_post": ("split_post", 1), "lpf_late0": ("lpf_late", 0),
             "lpf_late1": ("lpf_late", 1), "lpf_late2": ("lpf_late", 2)}[how]
    r, w = _flight(pkg, fmsig, 2, lag, setup), serial_flight
    assert _sorted(np.sort(r["recs"], order=["call_index", "channel", "bit_index"]))
    got = np.sort(r["recs"], order=["call_index", "channel", "bit_index"])
    assert len(got) == len(w["recs"]) and (got == w["recs"]).all()
    assert (r["quality"][0] == w["quality"][0]).all() and (r["quality"][-1] == w["quality"][-1]).all()
    assert len(r["groups"]) == len(w["groups"]) and (r["groups"] == w["groups"]).all()
    for a, a0 in zip(r["audio"], w["audio"]):
        assert a.shape == a0.shape and (_bits(a) == _bits(a0)).all()


# ---- 4. the benchmark's dispatch ------------------------------------------------------------------------------------
def _groups_from_records(recs):
    """per channel: a passing D record in state 1 or 2 completes a group of the last four passing words"""
    out = []
    order = np.lexsort((recs["bit_index"], recs["call_index"], recs["channel"]))
    last_c, words = -1, []
    for c, k, w, p, ss, st in zip(*(recs[f][order].tolist() for f in
                                    ("channel", "call_index", "word", "position", "status", "state"))):
        if c != last_c:
            last_c, words = c, []
        if ss == 2:
            words = []
            continue
        words.append(w)
        if st in (1, 2) and p == 3 and len(words) >= 4:
            out.append((c, k, tuple(words[-4:])))
    return out


def _dispatch_run(pkg, fmsig, Cn, calls=12):
    import torch
    gen = fmsig.DeviceGenerator([fmsig.channel_params(FS, c, noise_sigma=0.05 + 0.05 * (c % 5)) for c in range(Cn)])
    b = pkg.Batch(pkg.make_params(FS, -0.15 * FS, 48000.0, 15000.0, D), Cn, record_callbacks=False)
    b.set_concurrency(2)
    b.set_rds_blocks(2)
    st = torch.cuda.current_stream().cuda_stream
    a_stride = (b.max_audio_floats(N) + 7) // 8 * 8
    iq = [torch.empty((Cn, 2 * N), dtype=torch.float32, device="cuda") for _ in range(2)]
    out = torch.empty((Cn, a_stride), dtype=torch.float32, device="cuda")
    recs, groups = [], []
    for k in range(calls):
        gen.generate(iq[k % 2], k * N, N)
        b.process_device(iq[k % 2].data_ptr(), N, N, out.data_ptr(), a_stride, st)
        if k >= 1:
            r, lost = b.collect_rds_blocks(cap=1 << 20, lag=1, stream=st)
            assert lost == 0
            recs.append(r)
            groups.append(b.collect_rds_array(cap=1 << 18, stream=st, lag=1))
    b.wait(stream=st)
    torch.cuda.synchronize()
    recs.append(b.collect_rds_blocks(cap=1 << 20, stream=st)[0])
    groups.append(b.collect_rds_array(cap=1 << 18, stream=st))
    q = b.rds_quality()
    b.close()
    return np.concatenate(recs), np.concatenate(groups), q


def _self_consistent(recs, groups, q, Cn):
    assert len(recs) > Cn and _sorted(recs)
    # every record's status / word / corrected follows from its own raw / position / state under CheckBlock
    offset = np.array([0x3D8, 0x3D4, 0x25C, 0x258, 0x3CC])[recs["position"]]
    after, syn, pre, flips = spec.check_block_vec(recs["raw"], offset, recs["state"] == 2)
    status = np.where(syn != 0, 2, np.where(pre != 0, 1, 0))
    assert (status == recs["status"]).all() and (flips == recs["corrected"]).all()
    assert ((after >> 10) == recs["word"]).all()
    bs = recs["state"] == 0
    assert (recs["status"][bs] == 0).all() and (recs["position"][bs] == 0).all() and recs["state"].max() <= 2
    # the groups rebuilt from the records are the groups delivered
    g = np.sort(groups, order=["channel", "call_index"])
    want = [(int(c), int(k), tuple(int(v) for v in bl)) for c, k, bl in zip(g["channel"], g["call_index"], g["blocks"])]
    assert _groups_from_records(recs) == want and len(want) > 0
    # counter identities
    n_rec = np.bincount(recs["channel"], minlength=Cn)
    assert ((q["blocks"] + q["candidates"]) == n_rec).all()
    assert (q["groups"] == np.bincount(groups["channel"], minlength=Cn)).all()
    for f, m in (("candidates", recs["state"] == 0), ("corrected", recs["status"] == 1), ("failed", recs["status"] == 2),
                 ("sync_lost", (recs["status"] == 2) & (recs["state"] == 2)),
                 ("sync_acquired", (recs["status"] != 2) & (recs["state"] == 1) & (recs["position"] == 3))):
        assert (q[f] == np.bincount(recs["channel"][m], minlength=Cn)).all(), f
    last = np.zeros(Cn, np.int64)
    np.maximum.at(last, recs["channel"], recs["bit_index"])
    assert (last <= q["bits"]).all() and (q["bits"] > 0).all()


@pytest.mark.parametrize("Cn", [4160, 16384])
def test_the_benchmarks_dispatch(pkg, fmsig, Cn):
    recs, groups, q = _dispatch_run(pkg, fmsig, Cn)
    _self_consistent(recs, groups, q, Cn)
    # a 130-channel subset equals a small batch on the same inputs
    if Cn == 4160:
        small, _sg, sq = _dispatch_run(pkg, fmsig, 130)
        sub = recs[recs["channel"] < 130]
        assert len(sub) == len(small) and (sub == small).all() and (q[:130] == sq).all()
    else:  # a shell: global channel numbers out of both sub-batches
        assert recs["channel"].max() >= 8192 and (q["bits"][8192:] > 0).all()


# ---- 5. edits -------------------------------------------------------------------------------------------------------
def _retuned_spec(oracle, blocks, old_shift, new_shift, at, reset_at):
    """a slot retuned in front of call `at`: until then a decoder on old_shift, from there a decoder created with
    new_shift that received zeros until now -- the machine is replaced, the slot's counters run on"""
    old = oracle.OracleDecoder(FS, 0.0, 48000.0, 15000.0, D, table_size=TABLE, tuning_shift=int(old_shift))
    new = oracle.OracleDecoder(FS, 0.0, 48000.0, 15000.0, D, table_size=TABLE, tuning_shift=int(new_shift))
    s, z = spec.SyncSpec(0), spec.SyncSpec(0)
    for k, x in enumerate(blocks):
        if k == reset_at:
            new.reset()
            s.reset_machine()
        if k < at:
            old.process_stream(x)
            t = old.taps()
            s.call(k + 1, t["rds_mf"], t["rds_sync"])
            new.process_stream(np.zeros_like(x))
            t = new.taps()
            z.call(k + 1, t["rds_mf"], t["rds_sync"], 0)
            continue
        if k == at:
            s.replace_machine(z)
        new.process_stream(x)
        t = new.taps()
        s.call(k + 1, t["rds_mf"], t["rds_sync"])
    old.close()
    new.close()
    return s


def test_edits_restart_or_replace_the_machine_and_leave_the_counters(pkg, oracle, fmsig):
    caps = cases.captures(fmsig, "mixed")[:30]
    A, E = cases.SHIFT_A, cases.SHIFT_EMPTY
    b = pkg.Batch(_params(pkg), 4, tuning_shifts=np.array([A, A, E, A], np.int32), record_callbacks=False)
    b.enable_retune()
    b.set_capture_map(np.array([2, 2, 2, 0], np.uint32), cases.N_CAPTURES)
    b.set_rds_blocks(2)
    for k, x in enumerate(caps):
        if k == 8:
            b.reset_channels([0])
        if k == 12:
            b.retune([2], [A])            # from an empty step onto the station
        if k == 16:
            b.switch_captures([3], [2])   # all state carried over: nothing restarts
        if k == 22:
            b.reset()
        b.process_host_fmt(x)
    cap2 = [x[2] for x in caps]
    moved = [x[0] for x in caps[:16]] + cap2[16:]
    want = {0: cases.oracle_spec(oracle, cap2, A, "edits", resets=(8, 22))[0],
            1: cases.oracle_spec(oracle, cap2, A, "edits", resets=(22,))[0],
            2: _retuned_spec(oracle, cap2, E, A, 12, 22),
            3: cases.oracle_spec(oracle, moved, A, "edits-moved", resets=(22,))[0]}
    recs, lost = b.collect_rds_blocks()
    assert lost == 0 and len({w.quality() for w in want.values()}) == 4
    _same_records(recs, b.rds_quality(), want)
    b.close()


def _slot_specs(oracle, caps, decoders, lives):
    """Slots whose decoder is replaced in front of calls (an import, a load).  decoders: {name: (shift, capture of
    every call)}; lives: per slot [(first call, decoder name), ...].  Every decoder is an oracle decoder fed its own
    capture's rows from call 0; a slot's spec takes the taps of the decoder it is at that call, its machine replaced
    by that decoder's where the decoder changes -- and the slot's counters run on."""
    orc = {n: oracle.OracleDecoder(FS, 0.0, 48000.0, 15000.0, D, table_size=TABLE, tuning_shift=int(sh))
           for n, (sh, _c) in decoders.items()}
    shadow = {n: spec.SyncSpec(0) for n in decoders}  # the decoder's machine alone, wherever it lives
    slots = [spec.SyncSpec(0) for _ in lives]
    now = [None] * len(lives)
    for k, x in enumerate(caps):
        taps = {}
        for n, (_sh, cap_of) in decoders.items():
            orc[n].process_stream(x[cap_of[k]])
            t = orc[n].taps()
            taps[n] = (t["rds_mf"].copy(), t["rds_sync"].copy())
        for i, life in enumerate(lives):
            name = [n for first, n in life if first <= k][-1]
            if now[i] is not None and name != now[i]:
                slots[i].replace_machine(shadow[name])
            now[i] = name
            slots[i].call(k + 1, taps[name][0], taps[name][1])
        for n in decoders:
            shadow[n].call(k + 1, taps[n][0], taps[n][1], 0)
    for o in orc.values():
        o.close()
    return slots


def test_imports_and_loads_replace_the_machine_and_leave_the_counters(pkg, oracle, fmsig):
    """Decoders of a second batch (itself counting) imported in front of call 6; the state of a third batch loaded in
    front of call 12, with the records of calls 10-12 still queued: those are dropped like queued groups, the
    counters -- the slot's, not the decoder's, and no part of a blob -- run on, the mode stays, and everything
    collected afterwards is exact."""
    n_calls, A, B, E = 24, cases.SHIFT_A, cases.SHIFT_B, cases.SHIFT_EMPTY
    caps = cases.captures(fmsig, "mixed")[:n_calls]

    def batch(shifts, cmap):
        x = pkg.Batch(_params(pkg), len(shifts), tuning_shifts=np.array(shifts, np.int32), record_callbacks=False)
        x.set_capture_map(np.array(cmap, np.uint32), cases.N_CAPTURES)
        return x

    b = batch([A, A, B, E], [2, 2, 2, 2])
    src = batch([A, B], [0, 0])
    other = batch([A, B, A, B], [0, 0, 1, 1])
    b.set_rds_blocks(2)
    src.set_rds_blocks(1)  # its counters are its own slots': they do not travel
    got = []
    for k, x in enumerate(caps):
        if k == 6:
            b.import_channels([1, 3], src.export_channels([0, 1]))
        if k == 12:
            q0 = b.rds_quality()
            b.load_state(other.save_state())
            assert b.rds_blocks() == 2 and (b.rds_quality() == q0).all()
            r, lost = b.collect_rds_blocks()
            assert len(r) == 0 and lost == 0  # queued block records are dropped with the queued groups
        for y in (b, src, other):
            y.process_host_fmt(x)
        if k == 8:
            got.append(b.collect_rds_blocks()[0])  # calls 1-9; calls 10-12 stay queued until the load
    r, lost = b.collect_rds_blocks()
    assert lost == 0
    got.append(r)
    recs = np.concatenate(got)
    decoders = {"b0": (A, [2] * n_calls), "b1": (A, [2] * n_calls), "b2": (B, [2] * n_calls), "b3": (E, [2] * n_calls),
                "s0": (A, [0] * 6 + [2] * 18), "s1": (B, [0] * 6 + [2] * 18),  # an imported decoder reads the slot's capture
                "o0": (A, [0] * n_calls), "o1": (B, [0] * n_calls), "o2": (A, [1] * n_calls), "o3": (B, [1] * n_calls)}
    lives = [[(0, "b0"), (12, "o0")], [(0, "b1"), (6, "s0"), (12, "o1")], [(0, "b2"), (12, "o2")],
             [(0, "b3"), (6, "s1"), (12, "o3")]]
    want = _slot_specs(oracle, caps, decoders, lives)
    q = b.rds_quality()
    dropped = 0
    for c, w in enumerate(want):
        exp = w.records_array().copy()
        exp["channel"] = c
        gone = (exp["call_index"] >= 10) & (exp["call_index"] <= 12)
        dropped += int(gone.sum())
        exp = exp[~gone]
        have = recs[recs["channel"] == c]
        assert len(have) == len(exp) and (have == exp).all(), c
        assert tuple(int(v) for v in q[c]) == w.quality(), c  # (the dropped records were counted)
    assert (recs["call_index"] > 12).any() and (recs["call_index"] < 10).any()
    assert dropped > 0 and len(recs) == sum(int((recs["channel"] == c).sum()) for c in range(4))
    assert (other.rds_quality().view(np.uint32) == 0).all() and src.rds_quality()["bits"].min() > 0
    for y in (b, src, other):
        y.close()


# ---- 6. overflow ----------------------------------------------------------------------------------------------------
def test_a_full_queue_loses_records_and_nothing_else(pkg, oracle, fmsig):
    Cn = 130
    caps = cases.captures(fmsig, "mixed")[:10]
    stream_of = [c % len(cases.MIXED_STREAMS) for c in range(Cn)]
    cmap = np.array([cases.MIXED_STREAMS[s][0] for s in stream_of], np.uint32)
    shifts = np.array([cases.MIXED_STREAMS[s][1] for s in stream_of], np.int32)
    b = pkg.Batch(_params(pkg), Cn, tuning_shifts=shifts, record_callbacks=False)
    b.set_capture_map(cmap, cases.N_CAPTURES)
    b.set_rds_blocks(2, queue_records=64)
    with pytest.raises(pkg.FmdError):
        b.set_rds_blocks(2, queue_records=128)  # fixed by the first call that enabled mode 2
    b.set_rds_blocks(2, queue_records=64)
    for x in caps:
        b.process_host_fmt(x)  # ten calls, nothing collected: calls 9 and 10 append to the queues of calls 1 and 2
    want = {}
    for c in range(Cn):
        cap, shift = cases.MIXED_STREAMS[stream_of[c]]
        blocks = [x[cap] for x in caps]
        want[c] = cases.oracle_spec(oracle, blocks, shift, ("overflow", cap))[0]
    q = b.rds_quality()
    total = int((q["blocks"].astype(np.int64) + q["candidates"]).sum())
    assert total > 8 * 64  # (the case is an overflow)
    recs, lost = b.collect_rds_blocks(cap=100)  # ... and `out` is too small as well
    assert len(recs) == 100 and len(recs) + lost == total and _sorted(recs)
    for c in range(Cn):  # every returned record is a spec record; the counters are exact
        exp = want[c].records_array().copy()
        exp["channel"] = c
        got = recs[recs["channel"] == c]
        assert set(got.tolist()) <= set(exp.tolist()), c
        assert tuple(int(x) for x in q[c]) == want[c].quality(), c
    assert not b.take_rds_lost()  # no warning flag is touched
    again, lost = b.collect_rds_blocks()
    assert len(again) == 0 and lost == 0
    b.process_host_fmt(caps[0])  # the batch goes on
    q2 = b.rds_quality()
    recs, lost = b.collect_rds_blocks()
    assert len(recs) + lost == int((q2["blocks"].astype(np.int64) + q2["candidates"]).sum()) - total
    b.close()


# ---- 7. single decoder, surfaces, refusals ---------------------------------------------------------------------------
def test_a_single_decoder_and_the_refusals(pkg, oracle, fmsig):
    blocks = cases.plain_020(fmsig)[:20]
    dec = pkg.FmDecoder(FS, -0.7e6, 48000.0, 15000.0, D)
    ref = oracle.OracleDecoder(FS, -0.7e6, 48000.0, 15000.0, D)
    want = spec.SyncSpec(0)
    v = dec.batch_view()
    v.set_rds_blocks(2)
    for k, x in enumerate(blocks):
        a = dec.ProcessStream(x.view(np.complex64))
        a0 = ref.process_stream(x)
        assert (_bits(a) == _bits(a0)).all()
        t = ref.taps()
        want.call(k + 1, t["rds_mf"], t["rds_sync"])
    recs, lost = v.collect_rds_blocks()
    assert lost == 0 and len(recs) > 0
    _same_records(recs, v.rds_quality(), {0: want})
    L = pkg.lib()
    h = v._h
    assert L.fmd_batch_set_rds_blocks(h, 3, 0) < 0 and L.fmd_batch_set_rds_blocks(h, -1, 0) < 0
    assert v.rds_blocks() == 2  # a refusal leaves the mode
    one = np.zeros(1, pkg.RDS_BLOCK_DTYPE)
    assert L.fmd_batch_collect_rds_blocks(h, one.ctypes.data, 1, 5, None, None) < 0
    assert L.fmd_batch_collect_rds_blocks(h, None, 1, 0, None, None) < 0
    q = np.zeros(2, pkg.RDS_QUALITY_DTYPE)
    assert L.fmd_batch_read_rds_quality(h, 0, 2, q.ctypes.data) < 0
    assert L.fmd_batch_read_rds_quality(h, 1, 1, q.ctypes.data) < 0
    assert L.fmd_batch_read_rds_quality(h, 0, 1, None) < 0
    assert L.fmd_batch_read_rds_quality(h, 1, 0, q.ctypes.data) == 0
    v.set_rds_blocks(0)
    before = v.rds_quality().copy()
    dec.ProcessStream(blocks[0].view(np.complex64))
    assert (v.rds_quality() == before).all() and len(v.collect_rds_blocks()[0]) == 0
    dec.close()
    ref.close()
