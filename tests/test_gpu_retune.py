"""Retuning single channels of a running batch (fmd_batch_retune_channels, include/fmd.h), bit for bit.

A retuned channel must decode like an oracle decoder created with the new shift that received zeros of the same
call sizes before the edit (and every whole-batch reset); channels that were not edited must equal the same batch
run without edits.  Oracle decoders run only for the edited channels."""
import numpy as np
import pytest
import torch

from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

N = 65536
FS, D, T = 2.4e6, 11, 24  # tuner table of 24 entries: a shift step is 100 kHz


def _stations(fmsig):
    """A loud stereo + RDS station at -700 kHz, a quieter stereo one with another PI and PS at +500 kHz, a mono one
    at +100 kHz."""
    return [fmsig.default_params(FS, f_offset=-700e3, amp=0.3, noise_sigma=0.004, seed=91, pi=0x7011, ps="LOUD"),
            fmsig.default_params(FS, f_offset=500e3, amp=0.12, noise_sigma=0.004, seed=92, pi=0x7022, ps="OTHER"),
            fmsig.mono_params(FS, f_offset=100e3, amp=0.2, noise_sigma=0.004, seed=93)]


def _capture(stations, fmsig, blk):
    cap = np.zeros(2 * N, dtype=np.float32)
    for p in stations:
        cap += fmsig.generate_f32(p, blk * N, N)
    return cap


def _shift_of(f_offset):
    return -int(round(f_offset / 100e3))  # the station at f comes to 0 with shift -f / 100 kHz (tests/test_gpu_configs)


def _params(pkg):
    return pkg.make_params(FS, 0.0, 48000.0, 15000.0, D, table_size=T)


def _oracle(oracle, shift):
    return oracle.OracleDecoder(FS, 0.0, 48000.0, 15000.0, D, table_size=T, tuning_shift=int(shift))


def _bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _status_equal(sg, so):
    return (bool(sg.stereo_detected) == bool(so.stereo) and np.float32(sg.tuning_offset) == np.float32(so.tuning_offset)
            and np.float32(sg.interface_level) == np.float32(so.if_level)
            and np.float32(sg.pilot_level) == np.float32(so.pilot_level))


# 8 channels: 0 on the loud station, 1 on the other stereo one, 2 on the mono one, the rest on empty steps
SHIFTS0 = [7, -5, -1, -3, 0, 3, -7, 10]


def _host_run(pkg, caps, edits_at, enable=True, skip=-1, u8=False, taps_at=None):
    """Host-buffer calls on a shared capture; edits_at = {call: [(channels, shifts), ...]} applied before that call.
    Returns (batch, [audio per call], {channel: frame count before each call}, taps)"""
    b = pkg.Batch(_params(pkg), len(SHIFTS0), tuning_shifts=np.array(SHIFTS0, np.int32))
    if enable:
        b.enable_retune()
        b.debug_restart_skip(skip)
    if taps_at is not None:
        b.enable_taps(True)
    audio, nframes, taps = [], [], {}
    for k, cap in enumerate(caps):
        nframes.append({c: len(b.sink.frames.get(c, [])) for c in range(len(SHIFTS0))})
        for ch, sh in edits_at.get(k, []):
            b.retune(ch, sh)
        audio.append(b.process_host_u8(cap, shared=True) if u8 else b.process_host(cap.view(np.complex64), shared=True))
        if taps_at is not None and k == taps_at:
            taps = {name: b.tap(name, 0) for name in ("mono_rs", "stereo_rs", "rds_lpf", "rds_pll", "rds_mf")}
    return b, audio, nframes, taps


def _oracle_run(oracle, shift, caps, k, u8=False):
    """Zeros of the call sizes before call k, then the capture."""
    o = _oracle(oracle, shift)
    out = []
    for j, cap in enumerate(caps):
        if j < k:
            out.append(o.process_stream(np.zeros(2 * N, np.float32)))
        else:
            out.append(o.process_stream_u8(cap) if u8 else o.process_stream(cap))
    return o, out


def test_retune_shared_capture_bit_exact(pkg_fixture, oracle, fmsig):
    """(a) + (f): channel 0 leaves the loud stereo station for the mono one, channel 1 is retuned twice before the
    same call (the last shift counts), channel 2 restarts on its own station, channel 5 moves onto the loud one;
    audio of every call, the getters, the UECP frames and the PS name follow exactly at call k."""
    pkg = pkg_fixture
    st = _stations(fmsig)
    nblk, K = 9, 4
    caps = [_capture(st, fmsig, j) for j in range(nblk)]
    edits = {K: [([0, 1, 2], [_shift_of(100e3), -9, SHIFTS0[2]]), ([1, 5], [_shift_of(500e3), _shift_of(-700e3)])]}
    final = {0: _shift_of(100e3), 1: _shift_of(500e3), 2: SHIFTS0[2], 5: _shift_of(-700e3)}
    b, audio, nframes, _ = _host_run(pkg, caps, edits)
    ref, audio_ref, _, _ = _host_run(pkg, caps, {}, enable=False)
    for j in range(nblk):
        for c in range(len(SHIFTS0)):
            if c not in final or j < K:  # untouched channels and every call before the edit: as without edits
                assert _bits(audio[j][c], audio_ref[j][c]), (j, c)
    for c, s in final.items():
        o, out = _oracle_run(oracle, s, caps, K)
        for j in range(K, nblk):
            assert _bits(audio[j][c], out[j]), (c, j)
        assert _status_equal(b.status(c), o.status()), c
        assert b.status_call_index(c) == nblk
        assert b.sink.frames.get(c, [])[nframes[K][c]:] == o.uecp_frames(), c
        if o.channel_name().strip():
            assert b.sink.names.get(c) == o.channel_name(), c
    # the station moved: the getters of channel 0 are no longer those of the loud station
    assert np.float32(b.status(0).tuning_offset) != np.float32(ref.status(0).tuning_offset)
    assert np.float32(b.status(0).interface_level) != np.float32(ref.status(0).interface_level)
    for c in range(len(SHIFTS0)):
        if c not in final:
            sg, sr = b.status(c), ref.status(c)
            assert (sg.stereo_detected, np.float32(sg.tuning_offset), np.float32(sg.pilot_level)) == \
                (sr.stereo_detected, np.float32(sr.tuning_offset), np.float32(sr.pilot_level))
            assert b.sink.frames.get(c, []) == ref.sink.frames.get(c, [])
    b.close()
    ref.close()


def test_retune_u8_and_whole_batch_reset(pkg_fixture, oracle, fmsig):
    """(d): byte input; a whole-batch reset between the calls reaches the retuned channel as it reaches a decoder
    that was reset at the same boundary."""
    pkg = pkg_fixture
    p = fmsig.default_params(FS, f_offset=-300e3, amp=0.3, noise_sigma=0.004, seed=95, pi=0x7033)
    nblk, K = 7, 3
    caps = [fmsig.generate_u8(p, j * N, N) for j in range(nblk)]
    b = pkg.Batch(_params(pkg), 4, tuning_shifts=np.array([0, 1, 2, 3], np.int32))
    b.enable_retune()
    o = _oracle(oracle, 3)
    for j in range(nblk):
        if j == K:
            b.retune([2], [3])
        if j == 5:
            b.reset()
            o.reset()
        a = b.process_host_u8(caps[j], shared=True)
        r = o.process_stream_u8(caps[j]) if j >= K else o.process_stream(np.zeros(2 * N, np.float32))
        if j >= K:
            assert _bits(a[2], r), j
    assert _status_equal(b.status(2), o.status())
    b.close()


@pytest.mark.parametrize("lag", [1, 2, 3])
def test_retune_with_calls_in_flight(pkg_fixture, oracle, fmsig, lag):
    """(c): concurrency mode 2, outputs consumed `lag` calls late; the edit is made while earlier calls are still
    running.  Calls before k are those of the batch without edits; from k on the channel is the oracle's."""
    pkg = pkg_fixture
    st = _stations(fmsig)
    nblk, K, C = 8, 4, 256
    caps = [torch.from_numpy(_capture(st, fmsig, j)).cuda() for j in range(nblk)]
    shifts = np.resize(np.array(SHIFTS0, np.int32), C)
    edited = {0: _shift_of(500e3), 200: _shift_of(-700e3)}

    def run(edit):
        b = pkg.Batch(_params(pkg), C, tuning_shifts=shifts, record_callbacks=False)
        if edit:
            b.enable_retune()
        b.set_concurrency(2)
        a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
        audio = [torch.zeros((C, a_stride), dtype=torch.float32, device="cuda") for _ in range(nblk)]
        s = torch.cuda.current_stream().cuda_stream
        nf = []
        for j in range(nblk):
            if edit and j == K:
                b.retune(list(edited), list(edited.values()))
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
        keep = [c for c in range(C) if c not in edited or j < K]
        assert np.array_equal(got[j][keep].view(np.uint32), ref[j][keep].view(np.uint32)), j
    for c, s in edited.items():
        _, out = _oracle_run(oracle, s, [x.cpu().numpy() for x in caps], K)
        for j in range(K, nblk):
            assert _bits(got[j][c], out[j]), (lag, c, j)


def test_retune_across_sub_batches(pkg_fixture, oracle, fmsig):
    """(e): 16 384 channels run as two sub-batches; edits in both halves reach the right channels."""
    pkg = pkg_fixture
    st = _stations(fmsig)
    nblk, K, C = 5, 2, 16384
    caps = [torch.from_numpy(_capture(st, fmsig, j)).cuda() for j in range(nblk)]
    b = pkg.Batch(_params(pkg), C, tuning_shifts=np.resize(np.array(SHIFTS0, np.int32), C), record_callbacks=False)
    b.enable_retune()
    edited = {5: _shift_of(-700e3), 8191: _shift_of(100e3), 8192: _shift_of(500e3), 16383: _shift_of(-700e3)}
    a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
    audio = torch.zeros((nblk, C, a_stride), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    nf = []
    for j in range(nblk):
        if j == K:
            b.retune(list(edited), list(edited.values()))
        nf.append(b.process_device(caps[j].data_ptr(), 0, N, audio[j].data_ptr(), a_stride, s))
    b.wait(stream=s)
    torch.cuda.synchronize()
    got = [audio[j][:, :nf[j]].cpu().numpy() for j in range(nblk)]
    for c, sh in edited.items():
        o, out = _oracle_run(oracle, sh, [x.cpu().numpy() for x in caps], K)
        for j in range(K, nblk):
            assert _bits(got[j][c], out[j]), (c, j)
        assert _status_equal(b.status(c), o.status()), c
    # channels untouched by the edits: the ones with the same shift before the edit still agree with each other
    for j in range(nblk):
        assert np.array_equal(got[j][8].view(np.uint32), got[j][8192 + 8].view(np.uint32)), j
    b.close()


def test_retune_errors(pkg_fixture, fmsig):
    """(g): enable after the first call, a channel listed twice, out of range, retune without enabling."""
    pkg = pkg_fixture
    cap = _capture(_stations(fmsig), fmsig, 0)
    b = pkg.Batch(_params(pkg), 4, tuning_shifts=np.array([0, 1, 2, 3], np.int32))
    with pytest.raises(pkg.FmdError, match="not enabled"):
        b.retune([0], [1])
    b.process_host(cap.view(np.complex64), shared=True)
    with pytest.raises(pkg.FmdError, match="first call"):
        b.enable_retune()
    b.close()
    b = pkg.Batch(_params(pkg), 4, tuning_shifts=np.array([0, 1, 2, 3], np.int32))
    b.enable_retune()
    with pytest.raises(pkg.FmdError, match="twice"):
        b.retune([1, 1], [2, 3])
    with pytest.raises(pkg.FmdError, match="out of range"):
        b.retune([4], [2])
    with pytest.raises(pkg.FmdError):
        b.debug_restart_skip(8)
    b.retune([], [])  # nothing to do
    b.process_host(cap.view(np.complex64), shared=True)
    b.close()


REGIONS = ["state", "if_hist", "br", "mix", "halfband", "rds_lpf", "rds_mf", "audio_lpf"]


def test_restart_regions_have_teeth(pkg_fixture, oracle, fmsig):
    """(h): the restart leaving out any one carried region breaks parity of the retuned channel in the first call
    behind the edit (channel 0 leaves the loud stereo + RDS station for the other stereo one); leaving out none
    keeps it.  The region table is complete and nothing in it is padding."""
    pkg = pkg_fixture
    st = _stations(fmsig)
    nblk, K = 5, 3
    caps = [_capture(st, fmsig, j) for j in range(nblk)]
    s_new = _shift_of(500e3)
    o = _oracle(oracle, s_new)
    for j in range(K):
        o.process_stream(np.zeros(2 * N, np.float32))
    o.process_stream(caps[K])
    ot = o.taps()
    broken = {}
    for skip in [-1] + list(range(len(REGIONS))):
        b, audio, _, taps = _host_run(pkg, caps[:K + 1], {K: [([0], [s_new])]}, skip=skip, taps_at=K)
        same = _bits(audio[K][0], _oracle_run(oracle, s_new, caps[:K + 1], K)[1][K]) and \
            all(_bits(taps[n], ot[n].view(np.float32) if n == "rds_lpf" else ot[n])
                for n in ("mono_rs", "stereo_rs", "rds_pll", "rds_mf")) and \
            _bits(taps["rds_lpf"].view(np.float32), ot["rds_lpf"].view(np.float32))
        broken[REGIONS[skip] if skip >= 0 else "none"] = not same
        b.close()
    assert broken.pop("none") is False
    assert all(broken.values()), broken


@pytest.fixture(scope="module")
def pkg_fixture():
    return load_package()
