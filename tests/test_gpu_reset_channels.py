"""Resetting single channels of a running batch (fmd_batch_reset_channels, include/fmd.h), bit for bit.

A reset channel must decode like an oracle decoder that received the same inputs and reset() (cFmDecoder::Reset)
between call K-1 and call K; channels that were not listed must equal the same batch run without resets.  The RDS
low-pass and matched filter of a reset channel start their rings afresh while the batch's run on: the per-channel
ring origin is what keeps them exact, and the teeth test shows it."""
import numpy as np
import pytest
import torch

from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

N = 65536
FS, D, T = 2.4e6, 11, 24  # tuner table of 24 entries: a shift step is 100 kHz
RDS_TAPS = ("rds_lpf", "rds_pll", "rds_mf")


def _stations(fmsig):
    """A loud stereo + RDS station at -700 kHz, a quieter stereo one with another PI and PS at +500 kHz, a mono one
    at +100 kHz (the stations of tests/test_gpu_retune.py)."""
    return [fmsig.default_params(FS, f_offset=-700e3, amp=0.3, noise_sigma=0.004, seed=91, pi=0x7011, ps="LOUD"),
            fmsig.default_params(FS, f_offset=500e3, amp=0.12, noise_sigma=0.004, seed=92, pi=0x7022, ps="OTHER"),
            fmsig.mono_params(FS, f_offset=100e3, amp=0.2, noise_sigma=0.004, seed=93)]


def _capture(stations, fmsig, blk):
    cap = np.zeros(2 * N, dtype=np.float32)
    for p in stations:
        cap += fmsig.generate_f32(p, blk * N, N)
    return cap


def _shift_of(f_offset):
    return -int(round(f_offset / 100e3))


def _params(pkg, fs=FS, d=D, t=T, order=0):
    return pkg.make_params(fs, 0.0, 48000.0, 15000.0, d, table_size=t, if_filter_order=order)


def _oracle(oracle, shift, fs=FS, d=D, t=T, order=0):
    return oracle.OracleDecoder(fs, 0.0, 48000.0, 15000.0, d, table_size=t, if_filter_order=order,
                                tuning_shift=int(shift))


def _bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.complex64:
        a = a.view(np.float32)
    if b.dtype == np.complex64:
        b = b.view(np.float32)
    a, b = a.astype(np.float32, copy=False), b.astype(np.float32, copy=False)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _status_equal(sg, so):
    return (bool(sg.stereo_detected) == bool(so.stereo) and np.float32(sg.tuning_offset) == np.float32(so.tuning_offset)
            and np.float32(sg.interface_level) == np.float32(so.if_level)
            and np.float32(sg.pilot_level) == np.float32(so.pilot_level))


# 8 channels: 0 on the loud station, 1 on the other stereo one, 2 on the mono one, the rest on empty steps
SHIFTS0 = [7, -5, -1, -3, 0, 3, -7, 10]


def _host_run(pkg, caps, edits_at, enable=False, u8=False, taps_of=None, debug=None, keep_phase=False):
    """Host-buffer calls on a shared capture.  edits_at = {call: [("reset", channels) | ("retune", channels, shifts)
    | ("reset_all",)]} applied before that call, in order.  Returns (batch, [audio per call], [RDS taps of channel
    taps_of per call])."""
    b = pkg.Batch(_params(pkg), len(SHIFTS0), tuning_shifts=np.array(SHIFTS0, np.int32))
    if enable:
        b.enable_retune()
    for k, v in (debug or {}).items():
        b.debug_set(k, v)
    if keep_phase:
        b.debug_reset_keep_ring_phase(1)
    if taps_of is not None:
        b.enable_taps(True)
    audio, taps = [], []
    for k, cap in enumerate(caps):
        for e in edits_at.get(k, []):
            if e[0] == "reset":
                b.reset_channels(e[1])
            elif e[0] == "retune":
                b.retune(e[1], e[2])
            else:
                b.reset()
        audio.append(b.process_host_u8(cap, shared=True) if u8 else b.process_host(cap.view(np.complex64), shared=True))
        if taps_of is not None:
            taps.append({n: b.tap(n, taps_of) for n in RDS_TAPS})
    return b, audio, taps


def _oracle_run(oracle, shift, caps, resets=(), zeros_before=0, u8=False):
    """An oracle decoder on the same captures, reset() in front of every call in `resets`; zeros of the call sizes
    instead of the captures before call zeros_before (a retuned channel).  Returns (decoder, audio, RDS taps)."""
    o = _oracle(oracle, shift)
    out, taps = [], []
    for j, cap in enumerate(caps):
        if j in resets:
            o.reset()
        if j < zeros_before:
            out.append(o.process_stream(np.zeros(2 * N, np.float32)))
        else:
            out.append(o.process_stream_u8(cap) if u8 else o.process_stream(cap))
        t = o.taps()
        taps.append({n: t[n] for n in RDS_TAPS})
    return o, out, taps


def _ring_phases(oracle, taps, k):
    """The batch's RDS low-pass and matched-filter ring phases at the first sample of call k (the RDS-rate samples
    of the calls before it, mod the tap counts)."""
    o = _oracle(oracle, 0)
    n = sum(len(t["rds_mf"]) for t in taps[:k])
    return n % len(o.rds_lpf_taps()), n % len(o.rds_mf_taps())


@pytest.mark.parametrize("ring4", [1, 0])
def test_reset_shared_capture_bit_exact(pkg_fixture, oracle, fmsig, ring4):
    """Channels 0 (loud stereo + RDS), 1 (other stereo + RDS) and 5 (empty step) of one shared float capture are
    reset before call K = 12 of 28 (enough calls for UECP frames on both sides); the batch's RDS ring phases there
    are 15 of 75 (low-pass) and 8 of 44 (matched filter), both non-zero (asserted).  The reset channels follow the oracle that got reset() there -- audio of
    every call, getters, status call index, UECP frames and PS name, the RDS low-pass / PLL / matched-filter taps
    at K and K+1 bitwise; the other channels are those of the batch without resets.  The 8 channels are one wave
    of mixed origins.  ring4 = 0: the LDS form of the ring filters (k_ring_fir_org) instead of k_ring_fir4_org."""
    pkg = pkg_fixture
    st = _stations(fmsig)
    nblk, K = 28, 12
    caps = [_capture(st, fmsig, j) for j in range(nblk)]
    listed = [0, 1, 5]
    dbg = {"ring4": ring4}
    b, audio, taps = _host_run(pkg, caps, {K: [("reset", listed)]}, taps_of=0, debug=dbg)
    ref, audio_ref, _ = _host_run(pkg, caps, {}, debug=dbg)
    ph_lpf, ph_mf = _ring_phases(oracle, taps, K)
    assert ph_lpf != 0 and ph_mf != 0, (ph_lpf, ph_mf)
    for j in range(nblk):
        for c in range(len(SHIFTS0)):
            if c not in listed or j < K:
                assert _bits(audio[j][c], audio_ref[j][c]), (j, c)
    for c in listed:
        o, out, otaps = _oracle_run(oracle, SHIFTS0[c], caps, resets=(K,))
        for j in range(nblk):
            assert _bits(audio[j][c], out[j]), (c, j)
        assert _status_equal(b.status(c), o.status()), c
        assert b.status_call_index(c) == nblk
        assert b.sink.frames.get(c, []) == o.uecp_frames(), c
        if o.channel_name().strip():
            assert b.sink.names.get(c) == o.channel_name(), c
        if c == 0:
            for j in (K, K + 1):
                for n in RDS_TAPS:
                    assert _bits(taps[j][n], otaps[j][n]), (j, n)
    assert len(b.sink.frames.get(0, [])) > 0  # the loud station's groups did arrive
    for c in range(len(SHIFTS0)):
        if c not in listed:
            sg, sr = b.status(c), ref.status(c)
            assert (sg.stereo_detected, np.float32(sg.interface_level), np.float32(sg.pilot_level)) == \
                (sr.stereo_detected, np.float32(sr.interface_level), np.float32(sr.pilot_level))
            assert b.sink.frames.get(c, []) == ref.sink.frames.get(c, [])
    b.close()
    ref.close()


def test_reset_u8_twice_around_whole_batch_reset(pkg_fixture, oracle, fmsig):
    """Byte input: channel 2 is reset before calls 2 and 5, the whole batch before call 4."""
    pkg = pkg_fixture
    p = fmsig.default_params(FS, f_offset=-300e3, amp=0.3, noise_sigma=0.004, seed=95, pi=0x7033)
    nblk = 7
    caps = [fmsig.generate_u8(p, j * N, N) for j in range(nblk)]
    shifts = np.array([3, 1, 3, 2], np.int32)
    runs = {}
    for name, edits in (("edit", {2: [("reset", [2])], 4: [("reset_all",)], 5: [("reset", [2])]}),
                        ("ref", {4: [("reset_all",)]})):
        b = pkg.Batch(_params(pkg), 4, tuning_shifts=shifts)
        audio = []
        for j in range(nblk):
            for e in edits.get(j, []):
                b.reset_channels(e[1]) if e[0] == "reset" else b.reset()
            audio.append(b.process_host_u8(caps[j], shared=True))
        runs[name] = (b, audio)
    b, audio = runs["edit"]
    ref, audio_ref = runs["ref"]
    o, out, _ = _oracle_run(oracle, 3, caps, resets=(2, 4, 5), u8=True)
    for j in range(nblk):
        assert _bits(audio[j][2], out[j]), j
        for c in (0, 1, 3):
            assert _bits(audio[j][c], audio_ref[j][c]), (j, c)
    assert _status_equal(b.status(2), o.status())
    assert b.sink.frames.get(2, []) == o.uecp_frames()
    b.close()
    ref.close()


@pytest.mark.parametrize("lag", [1, 2, 3])
def test_reset_with_calls_in_flight(pkg_fixture, oracle, fmsig, lag):
    """Concurrency mode 2, outputs consumed `lag` calls late; the reset is made while earlier calls are still
    running.  Calls before K are those of the batch without resets; from K on the channels are the oracle's."""
    pkg = pkg_fixture
    st = _stations(fmsig)
    nblk, K, C_ = 8, 4, 256
    caps = [torch.from_numpy(_capture(st, fmsig, j)).cuda() for j in range(nblk)]
    shifts = np.resize(np.array(SHIFTS0, np.int32), C_)
    listed = [0, 200]

    def run(edit):
        b = pkg.Batch(_params(pkg), C_, tuning_shifts=shifts, record_callbacks=False)
        b.set_concurrency(2)
        a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
        audio = [torch.zeros((C_, a_stride), dtype=torch.float32, device="cuda") for _ in range(nblk)]
        s = torch.cuda.current_stream().cuda_stream
        nf = []
        for j in range(nblk):
            if edit and j == K:
                b.reset_channels(listed)
            nf.append(b.process_device(caps[j].data_ptr(), 0, N, audio[j].data_ptr(), a_stride, s))
            if j >= lag:
                b.wait(stream=s, lag=lag)
        b.wait(stream=s)
        torch.cuda.synchronize()
        out = [audio[j][:, :nf[j]].cpu().numpy() for j in range(nblk)]
        b.close()
        return out

    got, ref = run(True), run(False)
    for j in range(nblk):
        keep = [c for c in range(C_) if c not in listed or j < K]
        assert np.array_equal(got[j][keep].view(np.uint32), ref[j][keep].view(np.uint32)), j
    host_caps = [x.cpu().numpy() for x in caps]
    for c in listed:
        _, out, _ = _oracle_run(oracle, shifts[c], host_caps, resets=(K,))
        for j in range(nblk):
            assert _bits(got[j][c], out[j]), (lag, c, j)


def test_reset_across_sub_batches(pkg_fixture, oracle, fmsig):
    """16 384 channels run as two sub-batches.  Reset: 8191 and 8192 (both sides of the boundary), 16383, the whole
    wave 64..127 (one origin: the uniform form with a shifted phase) and channel 130 alone in its wave (mixed)."""
    pkg = pkg_fixture
    st = _stations(fmsig)
    nblk, K, C_ = 5, 3, 16384
    caps = [torch.from_numpy(_capture(st, fmsig, j)).cuda() for j in range(nblk)]
    shifts = np.resize(np.array(SHIFTS0, np.int32), C_)
    listed = [8191, 8192, 16383, 130] + list(range(64, 128))

    def run(edit):
        b = pkg.Batch(_params(pkg), C_, tuning_shifts=shifts, record_callbacks=False)
        a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
        audio = torch.zeros((nblk, C_, a_stride), dtype=torch.float32, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        nf = []
        for j in range(nblk):
            if edit and j == K:
                b.reset_channels(listed)
            nf.append(b.process_device(caps[j].data_ptr(), 0, N, audio[j].data_ptr(), a_stride, s))
        b.wait(stream=s)
        torch.cuda.synchronize()
        out = [audio[j][:, :nf[j]].cpu().numpy() for j in range(nblk)]
        status = {c: b.status(c) for c in listed}
        b.close()
        return out, status

    (got, status), (ref, _) = run(True), run(False)
    keep = np.ones(C_, bool)
    keep[listed] = False
    for j in range(nblk):
        assert np.array_equal(got[j][keep].view(np.uint32), ref[j][keep].view(np.uint32)), j
    host_caps = [x.cpu().numpy() for x in caps]
    by_shift = {}
    for c in listed:
        s = int(shifts[c])
        if s not in by_shift:
            by_shift[s] = _oracle_run(oracle, s, host_caps, resets=(K,))
        o, out, _ = by_shift[s]
        for j in range(nblk):
            assert _bits(got[j][c], out[j]), (c, j)
        assert _status_equal(status[c], o.status()), c


def test_reset_and_retune_in_order(pkg_fixture, oracle, fmsig):
    """With retuning enabled: a reset then a retune of channel 1 before call K is the retune alone; a retune then a
    reset of channel 2 is the retuned decoder reset at K; channel 3 reset at K and retuned at K+2 is the retuned
    decoder from K+2 on (the retune takes the ring origin back to the batch's phase)."""
    pkg = pkg_fixture
    st = _stations(fmsig)
    nblk, K = 8, 3
    caps = [_capture(st, fmsig, j) for j in range(nblk)]
    s1, s2, s3 = _shift_of(500e3), _shift_of(-700e3), _shift_of(-700e3)
    edits = {K: [("reset", [1]), ("retune", [1, 2], [s1, s2]), ("reset", [2, 3])], K + 2: [("retune", [3], [s3])]}
    b, audio, _ = _host_run(pkg, caps, edits, enable=True)
    ref, audio_ref, _ = _host_run(pkg, caps, {}, enable=True)
    o1, out1, _ = _oracle_run(oracle, s1, caps, zeros_before=K)
    o2, out2, _ = _oracle_run(oracle, s2, caps, zeros_before=K, resets=(K,))
    _, out3a, _ = _oracle_run(oracle, SHIFTS0[3], caps, resets=(K,))
    o3, out3b, _ = _oracle_run(oracle, s3, caps, zeros_before=K + 2)
    for j in range(nblk):
        assert _bits(audio[j][1], out1[j] if j >= K else audio_ref[j][1]), (1, j)
        assert _bits(audio[j][2], out2[j] if j >= K else audio_ref[j][2]), (2, j)
        assert _bits(audio[j][3], out3b[j] if j >= K + 2 else out3a[j]), (3, j)
        for c in (0, 4, 5, 6, 7):
            assert _bits(audio[j][c], audio_ref[j][c]), (c, j)
    for c, o in ((1, o1), (2, o2), (3, o3)):
        assert _status_equal(b.status(c), o.status()), c
    # the groups: the loud station on channel 2 from K on, through a group decoder reset at K
    assert b.sink.frames.get(2, [])[-len(o2.uecp_frames()):] == o2.uecp_frames()
    assert len(o2.uecp_frames()) > 0
    b.close()
    ref.close()


def test_reset_all_channels_equals_whole_batch_reset(pkg_fixture, oracle, fmsig):
    """reset_channels(every channel) before call K gives the bits of reset() before call K: audio, RDS taps,
    groups, getters (all channels share one origin: the uniform form with a shifted phase)."""
    pkg = pkg_fixture
    st = _stations(fmsig)
    nblk, K = 7, 3
    caps = [_capture(st, fmsig, j) for j in range(nblk)]
    allc = list(range(len(SHIFTS0)))
    runs = []
    for edit in ([("reset", allc)], [("reset_all",)]):
        b, audio, taps = _host_run(pkg, caps, {K: edit}, taps_of=0)
        runs.append((b, audio, taps))
    (b, audio, taps), (w, audio_w, taps_w) = runs
    for j in range(nblk):
        for c in allc:
            assert _bits(audio[j][c], audio_w[j][c]), (j, c)
        for n in RDS_TAPS:
            assert _bits(taps[j][n], taps_w[j][n]), (j, n)
    for c in allc:
        assert b.sink.frames.get(c, []) == w.sink.frames.get(c, []), c
        assert b.sink.names.get(c) == w.sink.names.get(c), c
        sb, sw = b.status(c), w.status(c)
        assert (sb.stereo_detected, np.float32(sb.interface_level), np.float32(sb.baseband_level), sb.rds_state) == \
            (sw.stereo_detected, np.float32(sw.interface_level), np.float32(sw.baseband_level), sw.rds_state), c
    assert len(b.sink.frames.get(0, [])) > 0
    b.close()
    w.close()


def test_reset_channels_errors(pkg_fixture, fmsig):
    """Out of range, listed twice, a null list; an empty list is nothing to do."""
    pkg = pkg_fixture
    cap = _capture(_stations(fmsig), fmsig, 0)
    b = pkg.Batch(_params(pkg), 4, tuning_shifts=np.array([0, 1, 2, 3], np.int32))
    with pytest.raises(pkg.FmdError, match="out of range"):
        b.reset_channels([4])
    with pytest.raises(pkg.FmdError, match="twice"):
        b.reset_channels([1, 2, 1])
    assert pkg.lib().fmd_batch_reset_channels(b._h, None, 1) == -1
    assert b"null" in pkg.lib().fmd_last_error()
    b.reset_channels([])
    b.process_host(cap.view(np.complex64), shared=True)
    b.reset_channels(np.array([3], np.uint32))
    b.process_host(cap.view(np.complex64), shared=True)
    b.close()


def test_reset_ring_origin_has_teeth(pkg_fixture, oracle, fmsig):
    """With fmd_batch_debug_reset_keep_ring_phase the reset channel keeps the batch's ring phase instead of its own
    origin: its RDS low-pass and matched-filter taps at K (phases 55 / 32, non-zero) then differ from the oracle's,
    while everything before K still agrees."""
    pkg = pkg_fixture
    st = _stations(fmsig)
    nblk, K = 5, 4
    caps = [_capture(st, fmsig, j) for j in range(nblk)]
    b, audio, taps = _host_run(pkg, caps, {K: [("reset", [0])]}, taps_of=0, keep_phase=True)
    _, out, otaps = _oracle_run(oracle, SHIFTS0[0], caps, resets=(K,))
    ph_lpf, ph_mf = _ring_phases(oracle, taps, K)
    assert ph_lpf != 0 and ph_mf != 0
    for j in range(K):
        assert _bits(audio[j][0], out[j]), j
    assert not _bits(taps[K]["rds_lpf"], otaps[K]["rds_lpf"])
    assert not _bits(taps[K]["rds_mf"], otaps[K]["rds_mf"])
    b.close()


@pytest.fixture(scope="module")
def pkg_fixture():
    return load_package()
