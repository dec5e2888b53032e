"""Audio as signed 16-bit PCM (FMD_PCM_S16, include/fmd.h), converted in the registers of the audio tail kernel.

The contract needs no tolerance: s = saturate_int16(round_half_even(x * 32768.0f)), NaN gives 0, where x is the float
sample the FMD_PCM_F32 call writes; x * 2^15 is exact in float32, so every sample has one right value.  pcm16() below
is that specification in numpy.  The expected value of every test is pcm16() of the CPU oracle's float audio
(cFmDecoder::ProcessStream, FmDecode.cpp:417-502) or -- where the channel count is beyond the oracle's reach -- of the
product's own float call, itself pinned to the oracle by the other tests; never of the S16 output itself.  Every
comparison is an equality of integers.
"""
import numpy as np
import pytest

from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

N = 65536
FILL = 0x5A5A


def pcm16(x):
    y = np.asarray(x, np.float32) * np.float32(32768.0)
    with np.errstate(invalid="ignore"):
        r = np.clip(np.rint(y), -32768.0, 32767.0)
    return np.where(np.isnan(y), 0, r).astype(np.int16)


def clipped(x):
    """samples whose rounded value has to be clamped (NaN is not one)"""
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(np.asarray(x, np.float32) * np.float32(32768))
        return (r > 32767) | (r < -32768)


def value_sets():
    """every tie (k + 0.5) / 32768 and every integer k / 32768, k = -32769 ... 32768; the contract's edge list, +-0,
    the smallest denormal, 1e30, NaN; 10^6 random 32-bit patterns as floats"""
    k = np.arange(-32769, 32769, dtype=np.float64)
    ties = ((k + 0.5) / 32768.0).astype(np.float32)
    ints = (k / 32768.0).astype(np.float32)
    edges = np.array([1.0, -1.0, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, 32767.5 / 32768, np.inf, -np.inf, 0.0, -0.0,
                      np.float32(1e-45), -np.float32(1e-45), 1e30, -1e30, np.nan, -np.nan, 32766.5 / 32768,
                      -32768.5 / 32768, -32767.5 / 32768, 3.4e38, -3.4e38], dtype=np.float32)
    rnd = np.random.default_rng(16).integers(0, 2 ** 32, 10 ** 6, dtype=np.uint64).astype(np.uint32).view(np.float32)
    return {"ties": ties, "integers": ints, "edges": edges, "random": rnd}


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _same_pcm(got, want_float, what):
    """got (int16) == pcm16(want_float), with the first differences in the message"""
    want = pcm16(want_float)
    assert got.dtype == np.int16 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (what, bad.size, [(int(i), int(got.reshape(-1)[i]), int(want.reshape(-1)[i]),
                                             float(np.asarray(want_float).reshape(-1)[i])) for i in bad[:6]])


def _station(fmsig, fs, over, **kw):
    """the default stereo + RDS station (saturates in the stereo lock's transient) or its over-deviated twin"""
    if over:
        kw["dev"] = 150e3
    return fmsig.default_params(fs, noise_sigma=0.005, **kw)


def _status_tuple(b, c):
    s = b.status(c)
    vals = (s.tuning_offset, s.interface_level, s.baseband_level, s.pilot_level) + tuple(b.audio_level(c))
    return (s.stereo_detected, s.rds_state) + tuple(int(np.float32(v).view(np.uint32)) for v in vals)


# ---------------------------------------------------------------------------------------------------------------
# 1. every value through the device build of the conversion

@pytest.mark.parametrize("name", ["ties", "integers", "edges", "random"])
def test_device_build_of_the_conversion_equals_pcm16(pkg, name):
    x = value_sets()[name]
    got, zero = pkg.debug_math(8, x)
    want = pcm16(x).astype(np.float32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (name, bad.size, [(float(x[i]), float(got[i]), float(want[i])) for i in bad[:8]])
    assert not zero.any()


# ---------------------------------------------------------------------------------------------------------------
# 2. single decoder

@pytest.mark.parametrize("fs,D,over", [(2.4e6, 11, False), (2.4e6, 11, True), (1.0e6, 4, True)],
                         ids=["default-2p4M", "overdeviated-2p4M", "overdeviated-1p0M"])
def test_single_decoder_equals_pcm16_of_the_oracle(pkg, oracle, fmsig, fs, D, over):
    """cFmDecoder surface: ProcessStreamToPcm16 == pcm16(oracle's ProcessStream) == pcm16(ProcessStream of a second
    decoder) over 40 calls; UECP frames, PS name and stereo flag equal.  The streams hold what makes the comparison
    bite: ties, saturated samples, L != R, and samples on which round-half-away, truncation and a scale of 32767
    each give another integer."""
    p = _station(fmsig, fs, over)
    o = oracle.OracleDecoder(fs, -0.15 * fs, 48000.0, 15000.0, D)
    d16 = pkg.FmDecoder(fs, -0.15 * fs, 48000.0, 15000.0, D)
    df = pkg.FmDecoder(fs, -0.15 * fs, 48000.0, 15000.0, D)
    refs = []
    for blk in range(40):
        x = fmsig.generate_f32(p, blk * N, N)
        ref = o.process_stream(x)
        a16 = d16.ProcessStreamToPcm16(x.view(np.complex64))
        af = df.ProcessStream(x.view(np.complex64))
        _same_pcm(a16, ref, "block %d against the oracle" % blk)
        _same_pcm(a16, af, "block %d against ProcessStream" % blk)
        refs.append(ref.copy())
    assert d16.sink.frames.get(0, []) == o.uecp_frames() == df.sink.frames.get(0, [])
    assert d16.sink.names.get(0) == o.channel_name()
    assert d16.StereoDetected() == bool(o.status().stereo) == df.StereoDetected()
    assert len(o.rds_groups()) > 10  # not silence
    # the data, from the oracle's floats
    x = np.concatenate(refs)
    y = x.astype(np.float64) * 32768.0  # exact
    want = pcm16(x).astype(np.int64)
    n_tie = int(((y - np.floor(y)) == 0.5).sum())
    n_sat = int(clipped(x).sum())
    away = np.clip(np.sign(y) * np.floor(np.abs(y) + 0.5), -32768, 32767).astype(np.int64)
    trunc = np.clip(np.trunc(y), -32768, 32767).astype(np.int64)
    s32767 = np.clip(np.rint(x.astype(np.float64) * 32767.0), -32768, 32767).astype(np.int64)
    differ = [int((v != want).sum()) for v in (away, trunc, s32767)]
    print("samples %d ties %d saturated %d; half-away / truncation / 32767 differ on %s" % (x.size, n_tie, n_sat, differ))
    assert n_tie >= 1 and n_sat >= 1
    assert (want[0::2] != want[1::2]).any()
    assert all(n >= 1 for n in differ), differ
    # the counter of the decoder's one-channel batch
    assert int(d16.batch_view().pcm_clipped()[0]) == n_sat
    assert int(df.batch_view().pcm_clipped()[0]) == 0


# ---------------------------------------------------------------------------------------------------------------
# 3. ragged tiles, row strides, nothing behind a row's samples

def test_ragged_calls_write_their_samples_and_nothing_else(pkg, oracle, fmsig):
    """Five channels with their own shifts through the device entry point, calls of 65 536 / 20 001 / 8192 / 33 333
    samples, rows 24 elements longer than needed and pre-filled: every sample is pcm16(oracle), every element behind
    a row's samples still holds the fill.  The calls' frame counts leave 0, 1, 2 and 3 frames behind the last group
    of four (asserted): the ragged tile's 8-byte, 4-byte and 8 + 4-byte stores all run."""
    seen = set()
    for n in (65536, 20001, 8192, 33333):
        seen |= _ragged_calls(pkg, oracle, fmsig, n)
    assert seen == {0, 1, 2, 3}, seen


def _ragged_calls(pkg, oracle, fmsig, n):
    import torch
    fs, D = 2.4e6, 11
    shifts = [10, -7, 0, 31, 10]
    Cn = len(shifts)
    ps = [fmsig.channel_params(fs, c) for c in range(Cn - 1)] + [_station(fmsig, fs, True)]
    os_ = [oracle.OracleDecoder(fs, 0.0, 48000.0, 15000.0, D, tuning_shift=s) for s in shifts]
    b = pkg.Batch(pkg.make_params(fs, -0.15 * fs, 48000.0, 15000.0, D), Cn, tuning_shifts=shifts)
    stride = (b.max_audio_floats(n) + 7) // 8 * 8 + 24
    n_al = (n + 1) // 2 * 2
    counts = set()
    for blk in range(5):
        x = np.zeros((Cn, 2 * n_al), np.float32)
        for c in range(Cn):
            x[c, :2 * n] = fmsig.generate_f32(ps[c], blk * n, n)
        d_iq = torch.from_numpy(x).cuda()
        d_out = torch.full((Cn, stride), FILL, dtype=torch.int16, device="cuda")
        nf = b.process_device(d_iq.data_ptr(), n_al, n, d_out.data_ptr(), stride, pcm=np.int16)
        torch.cuda.synchronize()
        a = d_out.cpu().numpy()
        counts.add(nf // 2 % 4)
        for c in range(Cn):
            ref = os_[c].process_stream(x[c, :2 * n])
            assert nf == ref.size
            _same_pcm(a[c, :nf], ref, (blk, c))
        assert (a[:, nf:] == FILL).all(), (blk, np.argwhere(a[:, nf:] != FILL)[:4])
    b.close()
    return counts


# ---------------------------------------------------------------------------------------------------------------
# 4. the format belongs to the call

@pytest.mark.parametrize("lag", [1, 2, 3])
def test_format_per_call_with_calls_in_flight(pkg, oracle, fmsig, lag):
    """Concurrency 2, calls consumed `lag` late, F32 and S16 output alternating into rotating buffers, float / byte /
    S16 input in turn: the S16 calls equal pcm16 of, and the F32 calls equal the bits of, a run of the same calls
    with float output throughout.  Status record and audio meter (its per-call mean and rms included) are compared
    wherever the pipeline is drained: every fourth call and the end in the runs with calls in flight, and after
    EVERY call in a second pair of runs that drains behind each call.  Channel 0 of the float run is pinned to the
    oracle."""
    import torch
    fs, D, C = 2.4e6, 11, 6
    ps = [_station(fmsig, fs, c % 2 == 1, seed=40 + c, pi=0x4200 + c) for c in range(C)]
    in_seq = [np.float32, np.uint8, np.int16]
    sizes = [N, 30001, N, 8193, N, 20001, N, N, 33333, N, 10007, N]
    inputs, start = [], 0
    for k, n in enumerate(sizes):
        dt = in_seq[k % 3]
        n_al = (n + 1) // 2 * 2
        x = np.zeros((C, 2 * n_al), dtype=dt)
        for c in range(C):
            if dt == np.uint8:
                x[c, :2 * n] = fmsig.generate_u8(ps[c], start, n)
            elif dt == np.int16:
                x[c, :2 * n] = np.clip(np.rint(fmsig.generate_f32(ps[c], start, n).astype(np.float64) * 32767),
                                       -32768, 32767).astype(np.int16)
            else:
                x[c, :2 * n] = fmsig.generate_f32(ps[c], start, n)
        start += n
        inputs.append((x, n, n_al))
    fmt_of = {np.float32: pkg.FMD_IQ_F32, np.uint8: pkg.FMD_IQ_U8, np.int16: pkg.FMD_IQ_S16}

    def run(mixed, drain_every=4):
        b = pkg.Batch(pkg.make_params(fs, -0.15 * fs, 48000.0, 15000.0, D), C, record_callbacks=False)
        b.set_concurrency(2)
        st = torch.cuda.current_stream().cuda_stream
        stride = (b.max_audio_floats(N) + 63) // 64 * 64
        ring = [(torch.zeros((C, stride), dtype=torch.float32, device="cuda"),
                 torch.zeros((C, stride), dtype=torch.int16, device="cuda")) for _ in range(lag + 1)]
        keep, audio, status = [], [None] * len(sizes), {}

        def consume(k):  # call k is complete: its buffer goes back into the rotation
            s16 = mixed and k % 2 == 1
            audio[k] = ring[k % (lag + 1)][1 if s16 else 0][:, :nfs[k]].cpu().numpy()

        nfs = []
        for k, (x, n, n_al) in enumerate(inputs):
            if k > lag:
                consume(k - lag - 1)
            s16 = mixed and k % 2 == 1
            d_iq = torch.from_numpy(x).cuda()
            keep.append(d_iq)
            out = ring[k % (lag + 1)][1 if s16 else 0]
            nfs.append(b.process_device(d_iq.data_ptr(), n_al, n, out.data_ptr(), stride, st,
                                        fmt=fmt_of[in_seq[k % 3]], pcm=np.int16 if s16 else np.float32))
            if k % drain_every == drain_every - 1 or k == len(sizes) - 1:
                b.wait(stream=st)
                torch.cuda.synchronize()
                status[k] = [_status_tuple(b, c) for c in range(C)]
            else:
                b.wait(stream=st, lag=lag)
                torch.cuda.current_stream().synchronize()
        for k in range(max(0, len(sizes) - lag - 1), len(sizes)):
            consume(k)
        groups = b.collect_rds_array(cap=65536, stream=st)
        clip = b.pcm_clipped()
        b.close()
        return audio, status, np.sort(groups, order=["channel", "call_index"]), clip

    fa, fstat, fg, fclip = run(False)
    ma, mstat, mg, mclip = run(True)
    o = oracle.OracleDecoder(fs, -0.15 * fs, 48000.0, 15000.0, D)
    want_clip = np.zeros(C, np.uint64)
    for k, (x, n, n_al) in enumerate(inputs):
        dt = in_seq[k % 3]
        f0 = x[0, :2 * n]
        f0 = oracle.convert_u8(f0) if dt == np.uint8 else f0.astype(np.float32) * np.float32(2.0 ** -15) \
            if dt == np.int16 else f0
        assert _bits_equal(fa[k][0], o.process_stream(f0)), k
        if k % 2 == 1:
            _same_pcm(ma[k], fa[k], k)
            want_clip += clipped(fa[k]).sum(axis=1).astype(np.uint64)
        else:
            assert ma[k].dtype == np.float32 and _bits_equal(ma[k], fa[k]), k
    assert sorted(fstat) == sorted(mstat) and len(fstat) >= 3
    assert fstat == mstat
    # the same calls drained one by one: the status record and the meter of every call
    fa1, fstat1, fg1, _ = run(False, drain_every=1)
    ma1, mstat1, mg1, mclip1 = run(True, drain_every=1)
    assert sorted(fstat1) == list(range(len(sizes))) == sorted(mstat1)
    assert fstat1 == mstat1
    assert all(fstat1[k] == fstat[k] for k in fstat)
    for k in range(len(sizes)):
        assert _bits_equal(fa1[k], fa[k]), k
        if k % 2 == 1:
            _same_pcm(ma1[k], fa[k], k)
    assert np.array_equal(mclip1, want_clip)
    assert len(fg) > 0 and np.array_equal(fg, mg)
    assert np.array_equal(mclip, want_clip) and want_clip.max() > 0 and not fclip.any()


def test_host_entry_point_takes_any_stride(pkg, oracle, fmsig):
    """fmd_batch_process_host_pcm copies rows: an odd stride and an unaligned pointer are fine, formats alternate."""
    import ctypes as C
    fs, D, Cn = 2.4e6, 11, 3
    ps = [_station(fmsig, fs, c == 1, seed=70 + c) for c in range(Cn)]
    refs = [oracle.OracleDecoder(fs, -0.15 * fs, 48000.0, 15000.0, D) for _ in range(Cn)]
    b = pkg.Batch(pkg.make_params(fs, -0.15 * fs, 48000.0, 15000.0, D), Cn)
    start = 0
    for k, n in enumerate([N, 20001, 8192, 33333, N]):
        x = np.stack([fmsig.generate_f32(ps[c], start, n) for c in range(Cn)])
        start += n
        want = [refs[c].process_stream(x[c]) for c in range(Cn)]
        if k % 2 == 0:
            stride = b.max_audio_floats(n) + 3  # odd
            buf = np.full(Cn * stride + 1, FILL, np.int16)
            out = buf[1:]  # 2-byte aligned only
            nf = C.c_uint()
            rc = pkg.lib().fmd_batch_process_host_pcm(b._h, x.ctypes.data, pkg.FMD_IQ_F32, n, n, out.ctypes.data,
                                                      pkg.FMD_PCM_S16, stride, C.byref(nf))
            assert rc >= 0, pkg.lib().fmd_last_error()
            rows = out.reshape(Cn, stride)
            for c in range(Cn):
                _same_pcm(rows[c, :nf.value], want[c], (k, c))
            assert (rows[:, nf.value:] == FILL).all() and buf[0] == FILL
        else:
            a = b.process_host_fmt(x, pcm=np.int16 if k == 1 else None)
            for c in range(Cn):
                if k == 1:
                    _same_pcm(a[c], want[c], (k, c))
                else:
                    assert _bits_equal(a[c], want[c]), (k, c)
    b.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. the benchmark's dispatch

def _dispatch(pkg, fmsig, pcm, C, shifts, rows, sizes, setup=None, edit=None, mode=2, lag=2, cmap=None, T=0):
    """One batch, device buffers, calls submitted back to back and consumed `lag` late like bench.py.  rows[k]:
    [G, 2 n] float IQ of call k (G = 1: one shared capture).  edit(b, k) runs in front of call k.  Returns the
    audio of every call, the status tuples of every channel at the end and the clip counters."""
    import torch
    fs, D = 2.4e6, 11
    b = pkg.Batch(pkg.make_params(fs, -0.15 * fs, 48000.0, 15000.0, D, table_size=T), C, tuning_shifts=shifts,
                  record_callbacks=False)
    b.set_concurrency(mode)
    if setup:
        setup(b)
    if cmap is not None:
        b.set_capture_map(cmap, rows[0].shape[0])
    st = torch.cuda.current_stream().cuda_stream
    stride = (b.max_audio_floats(N) + 63) // 64 * 64
    keep, outs, nfs = [], [], []
    for k, n in enumerate(sizes):
        if edit:
            edit(b, k)
        n_al = (n + 1) // 2 * 2
        x = np.zeros((rows[k].shape[0], 2 * n_al), np.float32)
        x[:, :2 * n] = rows[k]
        d_iq = torch.from_numpy(x).cuda()
        d_out = torch.zeros((C, stride), dtype=torch.int16 if pcm else torch.float32, device="cuda")
        keep.append(d_iq)
        outs.append(d_out)
        nfs.append(b.process_device(d_iq.data_ptr(), n_al if cmap is not None else 0, n, d_out.data_ptr(), stride, st,
                                    pcm=np.int16 if pcm else None))
        if k >= lag and mode == 2:
            b.wait(stream=st, lag=lag)
    b.wait(stream=st)
    torch.cuda.synchronize()
    audio = [outs[k][:, :nfs[k]].cpu().numpy() for k in range(len(sizes))]
    status = [_status_tuple(b, c) for c in range(0, C, max(1, C // 64))]
    clip = b.pcm_clipped()
    b.close()
    return audio, status, clip


def _both(pkg, fmsig, C, shifts, rows, sizes, **kw):
    """the float run and the S16 run of one scenario: every channel of every call, status and counters"""
    fa, fs_, fclip = _dispatch(pkg, fmsig, False, C, shifts, rows, sizes, **kw)
    sa, ss_, sclip = _dispatch(pkg, fmsig, True, C, shifts, rows, sizes, **kw)
    want = np.zeros(C, np.uint64)
    for k in range(len(sizes)):
        _same_pcm(sa[k], fa[k], k)
        want += clipped(fa[k]).sum(axis=1).astype(np.uint64)
    assert fs_ == ss_
    assert np.array_equal(sclip, want) and want.any() and not fclip.any()
    return fa, sa


def _shared_rows(fmsig, fs, sizes, over=False):
    p = _station(fmsig, fs, over)
    rows, start = [], 0
    for n in sizes:
        rows.append(fmsig.generate_f32(p, start, n)[None, :])
        start += n
    return rows


def _shifts(C):
    return np.array([(10, 9, 10, 11)[c % 4] for c in range(C)], np.int32)


@pytest.mark.parametrize("how", ["overlapped", "mode0", "profiling2"])
def test_dispatch_shared_capture(pkg, oracle, fmsig, how):
    """1030 channels on one shared capture with device buffers: overlapped calls (two-tile FIR beside the whole-CU
    serial stage), everything on the caller's stream (mode 0), and profiling level 2."""
    fs, D, C = 2.4e6, 11, 1030
    sizes = [N, 30001, N, 8193, N, N]
    rows, shifts = _shared_rows(fmsig, fs, sizes, over=True), _shifts(C)
    kw = {"overlapped": {}, "mode0": {"mode": 0}, "profiling2": {"setup": lambda b: b.set_profiling(2)}}[how]
    fa, sa = _both(pkg, fmsig, C, shifts, rows, sizes, **kw)
    for c in (0, 1, 3, C - 1):
        o = oracle.OracleDecoder(fs, 0.0, 48000.0, 15000.0, D, tuning_shift=int(shifts[c]))
        for k in range(len(sizes)):
            _same_pcm(sa[k][c], o.process_stream(rows[k][0]), (c, k))


def test_dispatch_shuffled_capture_map_with_a_switch(pkg, oracle, fmsig):
    """1024 channels on 4 captures through a shuffled capture map; three channels switch captures in front of call 2."""
    fs, D, C, G = 2.4e6, 11, 1024, 4
    sizes = [N, N, 30001, N, N]
    sts = [_station(fmsig, fs, g % 2 == 1, seed=300 + g, pi=0x7100 + g) for g in range(G)]
    rows, start = [], 0
    for n in sizes:
        rows.append(np.stack([fmsig.generate_f32(sts[g], start, n) for g in range(G)]))
        start += n
    shifts = _shifts(C)
    cmap = np.random.default_rng(7).permutation(C) % G
    moved = {0: int((cmap[0] + 1) % G), C - 1: int((cmap[C - 1] + 2) % G), 517: int((cmap[517] + 3) % G)}

    def edit(b, k):
        if k == 2:
            b.switch_captures(np.array(list(moved), np.uint32), np.array(list(moved.values()), np.uint32))

    fa, sa = _both(pkg, fmsig, C, shifts, rows, sizes, cmap=cmap, edit=edit)
    for c in (0, 5, 517, C - 1):
        o = oracle.OracleDecoder(fs, 0.0, 48000.0, 15000.0, D, tuning_shift=int(shifts[c]))
        for k in range(len(sizes)):
            g = moved[c] if (c in moved and k >= 2) else int(cmap[c])
            _same_pcm(sa[k][c], o.process_stream(rows[k][g]), (c, k))


def test_dispatch_retune_and_reset_in_front_of_a_call(pkg, oracle, fmsig):
    """1024 channels, retuning enabled (the silent twin's audio stays float): two channels are retuned and two reset
    in front of call 2, with calls in flight."""
    fs, D, C = 2.4e6, 11, 1024
    sizes = [N, N, N, 30001, N]
    rows, shifts = _shared_rows(fmsig, fs, sizes, over=True), _shifts(C)
    retuned, reset = {3: 10, 700: 9}, [5, 900]

    def edit(b, k):
        if k == 2:
            b.retune(list(retuned), list(retuned.values()))
            b.reset_channels(reset)

    fa, sa = _both(pkg, fmsig, C, shifts, rows, sizes, setup=lambda b: b.enable_retune(), edit=edit)
    for c in (0, 3, 5, 900):
        sh = retuned.get(c, int(shifts[c]))
        o = oracle.OracleDecoder(fs, 0.0, 48000.0, 15000.0, D, tuning_shift=sh)
        for k in range(len(sizes)):
            if k == 2 and c in reset:
                o.reset()
            if k < 2 and c in retuned:  # a decoder of the new shift that received zeros until now
                o.process_stream(np.zeros(2 * sizes[k], np.float32))
                continue
            _same_pcm(sa[k][c], o.process_stream(rows[k][0]), (c, k))


def test_dispatch_16448_channels_as_sub_batches(pkg, oracle, fmsig):
    """16 448 channels = a shell over three sub-batches: every sub-batch's rows start ch0 * stride int16 elements
    into the caller's buffer."""
    fs, D, C = 2.4e6, 11, 16448
    sizes = [N, 30001, N]
    rows, shifts = _shared_rows(fmsig, fs, sizes, over=True), _shifts(C)
    fa, sa = _both(pkg, fmsig, C, shifts, rows, sizes)
    for c in (0, 8191, 8193, C - 1):
        o = oracle.OracleDecoder(fs, 0.0, 48000.0, 15000.0, D, tuning_shift=int(shifts[c]))
        for k in range(len(sizes)):
            _same_pcm(sa[k][c], o.process_stream(rows[k][0]), (c, k))


# ---------------------------------------------------------------------------------------------------------------
# 6. the saturation counter

def test_pcm_clipped_is_the_running_count(pkg, fmsig):
    """Four channels holding both stations, 40 calls: pcm_clipped() equals the running numpy count over the float
    audio of the S16 calls (a second batch's float calls), F32 calls in between add nothing, reset() and
    reset_channels() clear nothing, and the float batch's counters stay zero."""
    fs, D, Cn = 2.4e6, 11, 4
    ps = [_station(fmsig, fs, c % 2 == 1, seed=80 + c) for c in range(Cn)]
    b = pkg.Batch(pkg.make_params(fs, -0.15 * fs, 48000.0, 15000.0, D), Cn)
    bf = pkg.Batch(pkg.make_params(fs, -0.15 * fs, 48000.0, 15000.0, D), Cn)
    assert not b.pcm_clipped().any()
    run = np.zeros(Cn, np.uint64)
    for blk in range(40):
        if blk == 20:
            b.reset()
            bf.reset()
            assert np.array_equal(b.pcm_clipped(), run)
        if blk == 30:
            b.reset_channels([1, 2])
            bf.reset_channels([1, 2])
            assert np.array_equal(b.pcm_clipped(), run)
        x = np.stack([fmsig.generate_f32(ps[c], blk * N, N) for c in range(Cn)])
        af = bf.process_host_fmt(x)
        if blk % 4 == 3:  # a float call in between
            assert _bits_equal(b.process_host_fmt(x), af), blk
            assert np.array_equal(b.pcm_clipped(), run), blk
            continue
        _same_pcm(b.process_host_fmt(x, pcm=np.int16), af, blk)
        run += clipped(af).sum(axis=1).astype(np.uint64)
        if blk % 5 == 0 or blk > 36:
            assert np.array_equal(b.pcm_clipped(), run), blk
    assert np.array_equal(b.pcm_clipped(), run) and run.min() > 0 and run[1] > run[0]
    assert not bf.pcm_clipped().any()
    one = np.zeros(2, np.uint64)
    pkg._check(pkg.lib().fmd_batch_read_pcm_clipped(b._h, 1, 2, one.ctypes.data))
    assert np.array_equal(one, run[1:3])
    with pytest.raises(pkg.FmdError, match="out of range"):
        pkg._check(pkg.lib().fmd_batch_read_pcm_clipped(b._h, 3, 2, one.ctypes.data))
    b.close()
    bf.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. alignment

def test_device_entry_refuses_misaligned_s16_rows(pkg, fmsig):
    import torch
    fs, D = 2.4e6, 11
    b = pkg.Batch(pkg.make_params(fs, -0.15 * fs, 48000.0, 15000.0, D), 2)
    x = np.stack([fmsig.generate_f32(_station(fmsig, fs, False), 0, N)] * 2)
    iq = torch.from_numpy(x).cuda()
    stride = (b.max_audio_floats(N) + 7) // 8 * 8
    audio = torch.zeros(2 * 4 * (stride + 16), dtype=torch.uint8, device="cuda")
    assert audio.data_ptr() % 16 == 0
    with pytest.raises(pkg.FmdError, match="fmd error -1: .*16-byte aligned"):
        b.process_device(iq.data_ptr(), N, N, audio.data_ptr() + 8, stride, pcm=np.int16)
    with pytest.raises(pkg.FmdError, match="fmd error -1: .*multiple of 8"):
        b.process_device(iq.data_ptr(), N, N, audio.data_ptr(), stride + 2, pcm=np.int16)
    assert len(pkg.lib().fmd_last_error().split()) >= 5
    # the same pointer and stride are fine for float output, and the batch is still usable for S16
    nf = b.process_device(iq.data_ptr(), N, N, audio.data_ptr() + 8, stride + 2, pcm=np.float32)
    torch.cuda.synchronize()
    f = audio[8:8 + 4 * (2 * (stride + 2))].cpu().numpy().view(np.float32).reshape(2, stride + 2)[:, :nf]
    b2 = pkg.Batch(pkg.make_params(fs, -0.15 * fs, 48000.0, 15000.0, D), 2)
    assert _bits_equal(f, b2.process_host_fmt(x))
    out = torch.zeros((2, stride), dtype=torch.int16, device="cuda")
    nf = b.process_device(iq.data_ptr(), N, N, out.data_ptr(), stride, pcm=np.int16)
    torch.cuda.synchronize()
    _same_pcm(out[:, :nf].cpu().numpy(), b2.process_host_fmt(x), "after the refusals")
    b.close()
    b2.close()
