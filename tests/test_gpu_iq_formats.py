"""Signed 8- and 16-bit IQ (FMD_IQ_S8 / FMD_IQ_S16, include/fmd.h) converted inside the IF kernel.

The contract needs no tolerance: v * 2^-7 and v * 2^-15 are exact in float32, so a call with integer input gives the
same bits, in every output, as the float call on the block converted on the host with
v.astype(float32) * float32(2**-7 | 2**-15).  The expected value of every test is therefore the CPU oracle
(cFmDecoder::ProcessStream, FmDecode.cpp:417-502) -- or the product's float path, itself pinned to the oracle by the
other tests -- on the host-converted block, and every comparison is equality of the float bits.

Test signals: fmsig.generate_f32 (stereo + RDS stations) quantised here with round(x * 32767) / round(x * 127),
clipped to the integer range.
"""
from importlib import import_module

import numpy as np
import pytest

from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

N = 65536
DTYPES = [np.int8, np.int16]
IDS = ["s8", "s16"]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _quant(x, dt):
    """float IQ in [-1, 1] -> integer IQ of dtype dt: round(x * 32767) / round(x * 127), clipped"""
    info = np.iinfo(dt)
    return np.clip(np.rint(np.asarray(x, np.float64) * (32767 if dt == np.int16 else 127)), info.min,
                   info.max).astype(dt)


def _to_f32(q):
    """the contract's host conversion"""
    q = np.asarray(q)
    return q.astype(np.float32) * np.float32(2.0 ** -15 if q.dtype == np.int16 else 2.0 ** -7)


def _fmt(pkg, dt):
    return {np.dtype(np.int8): pkg.FMD_IQ_S8, np.dtype(np.int16): pkg.FMD_IQ_S16, np.dtype(np.uint8): pkg.FMD_IQ_U8,
            np.dtype(np.float32): pkg.FMD_IQ_F32}[np.dtype(dt)]


def _every_value_block(dt, rng):
    """S16: all 65 536 values on I and a permutation of them on Q; S8: all 256 x 256 (I, Q) pairs, shuffled"""
    buf = np.empty(2 * N, dtype=dt)
    if dt == np.int16:
        buf[0::2] = np.arange(-32768, 32768).astype(np.int16)[rng.permutation(N)]
        buf[1::2] = np.arange(-32768, 32768).astype(np.int16)[rng.permutation(N)]
    else:
        v = np.arange(-128, 128).astype(np.int8)
        buf[0::2] = np.tile(v, N // 256)
        buf[1::2] = np.repeat(v, N // 256)
        buf = buf.reshape(-1, 2)[rng.permutation(N)].reshape(-1)
    return buf


# ---------------------------------------------------------------------------------------------------------------
# every value

@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_every_integer_value_converts_exactly(pkg, oracle, dt):
    """The demodulator input tap (tuned, filtered, decimated) only equals the oracle's on the converted block if
    every one of the values converts exactly; two calls (the second starts from the first's delay line)."""
    fs, D = 2.4e6, 11
    buf = _every_value_block(dt, np.random.default_rng(5))
    assert np.unique(buf[0::2]).size == (65536 if dt == np.int16 else 256)
    o = oracle.OracleDecoder(fs, -0.15 * fs, 48000.0, 15000.0, D)
    b = pkg.Batch(pkg.make_params(fs, -0.15 * fs, 48000.0, 15000.0, D), 1)
    b.enable_taps()
    for _ in range(2):
        ref = o.process_stream(_to_f32(buf))
        a = b.process_host_fmt(buf, shared=True)
        assert _bits_equal(b.tap("demod").view(np.float32), o.taps()["demod"].view(np.float32))
        assert _bits_equal(a[0], ref)
    b.close()


def test_teeth_byte_swapped_s16_differs_from_the_oracle(pkg, oracle):
    """The comparison above has teeth: the product fed the byte-swapped array (what a big-endian file read as host
    order would be) does not give the oracle's tap on the converted block."""
    fs, D = 2.4e6, 11
    buf = _every_value_block(np.int16, np.random.default_rng(5))
    o = oracle.OracleDecoder(fs, -0.15 * fs, 48000.0, 15000.0, D)
    b = pkg.Batch(pkg.make_params(fs, -0.15 * fs, 48000.0, 15000.0, D), 1)
    b.enable_taps()
    o.process_stream(_to_f32(buf))
    b.process_host_fmt(buf.byteswap(), shared=True)
    assert not _bits_equal(b.tap("demod").view(np.float32), o.taps()["demod"].view(np.float32))
    b.close()


# ---------------------------------------------------------------------------------------------------------------
# single decoder

@pytest.mark.parametrize("fs,D", [(2.4e6, 11), (1.0e6, 4)])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_single_decoder_equals_convert_then_process(pkg, oracle, fmsig, dt, fs, D):
    """cFmDecoder surface: ProcessStreamS8 / S16 == the oracle's ProcessStream on the converted blocks, audio bit for
    bit, UECP frames and PS name identical; and equal to the product's own float path."""
    p = fmsig.default_params(fs, noise_sigma=0.005)
    o = oracle.OracleDecoder(fs, -0.15 * fs, 48000.0, 15000.0, D)
    di = pkg.FmDecoder(fs, -0.15 * fs, 48000.0, 15000.0, D)
    df = pkg.FmDecoder(fs, -0.15 * fs, 48000.0, 15000.0, D)
    call = di.ProcessStreamS16 if dt == np.int16 else di.ProcessStreamS8
    for blk in range(40):
        q = _quant(fmsig.generate_f32(p, blk * N, N), dt)
        x = _to_f32(q)
        a_ref = o.process_stream(x)
        a_i = call(q)
        a_f = df.ProcessStream(x.view(np.complex64))
        assert _bits_equal(a_i, a_ref), "block %d" % blk
        assert _bits_equal(a_i, a_f), "block %d" % blk
    assert di.sink.frames.get(0, []) == o.uecp_frames()
    assert di.sink.names.get(0) == o.channel_name()
    assert di.StereoDetected() == bool(o.status().stereo)
    assert len(o.rds_groups()) > 10  # not silence


# ---------------------------------------------------------------------------------------------------------------
# ragged blocks, tuner shifts, the level meter

@pytest.mark.parametrize("n", [65536, 20001, 8192, 33333])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_ragged_blocks_and_shifts(pkg, oracle, fmsig, dt, n):
    """Five channels with their own tuner shifts, block lengths that are not multiples of the pair load (the
    kernel's sample-by-sample tail), stage tap and audio bit for bit, interface_level of every channel (k_if_level)."""
    fs, D = 2.4e6, 11
    shifts = [10, -7, 0, 31, 10]
    Cn = len(shifts)
    ps = [fmsig.channel_params(fs, c) for c in range(Cn)]
    os_ = [oracle.OracleDecoder(fs, 0.0, 48000.0, 15000.0, D, tuning_shift=s) for s in shifts]
    b = pkg.Batch(pkg.make_params(fs, -0.15 * fs, 48000.0, 15000.0, D), Cn, tuning_shifts=shifts)
    b.enable_taps()
    for blk in range(6):
        q = np.stack([_quant(fmsig.generate_f32(ps[c], blk * n, n), dt) for c in range(Cn)])
        a = b.process_host_fmt(q)
        for c in range(Cn):
            a_ref = os_[c].process_stream(_to_f32(q[c]))
            assert _bits_equal(b.tap("demod", c).view(np.float32), os_[c].taps()["demod"].view(np.float32)), (blk, c)
            assert _bits_equal(a[c], a_ref), (blk, c)
    for c in range(Cn):
        assert np.float32(os_[c].status().if_level) == np.float32(b.status(c).interface_level), c
    b.close()


# ---------------------------------------------------------------------------------------------------------------
# every IF kernel form

def _run_stations(pkg, oracle, fmsig, dt, fs, D, C, sizes, order=0, table=0, K=8, lag=2, setup=None):
    """K distinct stations repeated over C channels (channel c carries station c % K), device calls of the given
    sizes submitted back to back in concurrency 2 and consumed `lag` calls late, like bench.py: the first channel of
    every station against the oracle on the converted block, all the others against their twin."""
    import torch
    ps = [fmsig.default_params(fs, noise_sigma=0.01, seed=31 + s, pi=0x3100 + s) for s in range(K)]
    refs = [oracle.OracleDecoder(fs, -0.15 * fs, 48000.0, 15000.0, D, table_size=table, if_filter_order=order)
            for _ in range(K)]
    b = pkg.Batch(pkg.make_params(fs, -0.15 * fs, 48000.0, 15000.0, D, table_size=table, if_filter_order=order), C,
                  record_callbacks=False)
    b.set_concurrency(2)
    if setup:
        setup(b)
    st = torch.cuda.current_stream().cuda_stream
    a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
    idx = torch.arange(C, device="cuda") % K
    base, bufs, outs, nfs, start = [], [], [], [], 0
    for k, n in enumerate(sizes):
        n_al = (n + 1) // 2 * 2  # channel stride: a whole number of sample pairs
        q = np.zeros((K, 2 * n_al), dtype=dt)
        for s in range(K):
            q[s, :2 * n] = _quant(fmsig.generate_f32(ps[s], start, n), dt)
        start += n
        base.append(q[:, :2 * n])
        d_iq = torch.from_numpy(q).cuda()[idx].contiguous()
        d_out = torch.zeros((C, a_stride), dtype=torch.float32, device="cuda")
        bufs.append(d_iq)
        outs.append(d_out)
        nfs.append(b.process_device(d_iq.data_ptr(), n_al, n, d_out.data_ptr(), a_stride, st, fmt=_fmt(pkg, dt)))
        if k >= lag:
            b.wait(stream=st, lag=lag)
    b.wait(stream=st)
    torch.cuda.synchronize()
    for k in range(len(sizes)):
        a = outs[k][:, :nfs[k]].cpu().numpy()
        for s in range(K):
            r = refs[s].process_stream(_to_f32(base[k][s]))
            assert _bits_equal(a[s], r), (k, s)
            twins = a[s::K]
            assert np.array_equal(twins.view(np.uint32), np.broadcast_to(a[s], twins.shape).view(np.uint32)), (k, s)
    for s in range(K):
        so, sg = refs[s].status(), b.status(s)
        assert sg.stereo_detected == so.stereo
        for f_o, f_g in ((so.if_level, sg.interface_level), (so.baseband_level, sg.baseband_level),
                         (so.pilot_level, sg.pilot_level), (so.tuning_offset, sg.tuning_offset)):
            assert np.float32(f_o) == np.float32(f_g), s
    b.close()


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_1030_channels_overlapped_whole_cu_form(pkg, oracle, fmsig, dt):
    """1030 channels with overlapped calls: the two-tile FIR workgroups beside the whole-CU serial stage, channel
    count not a multiple of 8 (blocks channel-major)."""
    _run_stations(pkg, oracle, fmsig, dt, 2.4e6, 11, 1030, [N, 10007, N, 33001])


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_benchmarked_dispatch_at_4096_channels(pkg, oracle, fmsig, dt):
    """The form bench.py runs (k_if_fir_mt3, XCD-aware block mapping, two outputs per lane) at 4096 channels, on full
    and ragged calls."""
    _run_stations(pkg, oracle, fmsig, dt, 2.4e6, 11, 4096, [N, 30001, N, 8193])


@pytest.mark.parametrize("ro", [3, 1], ids=["3-per-lane", "1-per-lane"])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_other_two_tile_forms(pkg, oracle, fmsig, dt, ro):
    """k_if_fir_mt3 with three outputs per lane and k_if_fir_mt (one output per lane, two tiles per workgroup)."""
    _run_stations(pkg, oracle, fmsig, dt, 2.4e6, 11, 1024, [N, 10007, 150, 65535, N],
                  setup=lambda b: b.debug_set("fir_ro", ro))


@pytest.mark.parametrize("nt", [3, 4, 8])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_k_if_fir_mt_tile_counts(pkg, oracle, fmsig, dt, nt):
    """k_if_fir_mt with 3, 4 and 8 tiles per workgroup ("fir_nt" of fmd_batch_debug_set)."""
    _run_stations(pkg, oracle, fmsig, dt, 2.4e6, 11, 1024, [N, 10007, N],
                  setup=lambda b: b.debug_set("fir_nt", nt))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_config5_long_filter_on_its_benchmarked_dispatch(pkg, oracle, fmsig, dt):
    """BASELINE configs[4] (4096-tap filter, 10 MS/s, D = 46) the way bench.py runs it: channel count a multiple of 8
    and >= 1024 (XCD-aware mapping, 256 outputs per workgroup, hand-scheduled tap loop), overlapped calls."""
    _run_stations(pkg, oracle, fmsig, dt, 10e6, 46, 1032, [N, 40001, N], order=4096)


@pytest.mark.parametrize("fs,D,order", [(2.4e6, 11, 2048), (9.6e6, 44, 2048), (1.8e6, 8, 1500), (1.0e6, 4, 1500),
                                        (1.4e6, 6, 1024)],
                         ids=["odd-D", "4x-odd-D", "8x-D", "D4", "2x-odd-D"])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_long_filter_tap_loops_of_every_window_layout(pkg, oracle, fmsig, dt, fs, D, order):
    """The hand-scheduled long-filter tap loops behind every window layout (plain window read 8 and 16 bytes at a
    time, two and four regions, the 16-byte-read region forms), full and ragged blocks."""
    _run_stations(pkg, oracle, fmsig, dt, fs, D, 16, [N, 40001, 12288], order=order, K=2)


@pytest.mark.parametrize("fs,D", [(1.0e6, 4), (1.4e6, 6), (3.5e6, 16)], ids=["D4", "D6", "D16"])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_even_decimation_deinterleaved_window(pkg, oracle, fmsig, dt, fs, D):
    """Even D with the short filter: the de-interleaved window (E > 0), a pair's two samples in neighbouring regions."""
    _run_stations(pkg, oracle, fmsig, dt, fs, D, 24, [N, 20001, 33333, N], K=3)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_cic_rate(pkg, oracle, fmsig, dt):
    """6.4 MS/s, D = 1: the baseband rate at which the RDS decimator starts with k_cic3; the IF stage at D = 1."""
    fs, D = 6.4e6, 1
    p = fmsig.default_params(fs, noise_sigma=0.01, seed=27)
    o = oracle.OracleDecoder(fs, -0.15 * fs, 48000.0, 15000.0, D)
    b = pkg.Batch(pkg.make_params(fs, -0.15 * fs, 48000.0, 15000.0, D), 2)
    b.enable_taps()
    start = 0
    for k, n in enumerate([32000, 20000, 4000, 32000, 2048, 32000]):
        q = _quant(fmsig.generate_f32(p, start, n), dt)
        start += n
        ref = o.process_stream(_to_f32(q))
        a = b.process_host_fmt(np.stack([q, q]))
        t = o.taps()
        for name in ("demod", "baseband", "rds_lpf", "rds_mf"):
            assert _bits_equal(b.tap(name, 1).view(np.float32), t[name].view(np.float32)), (k, n, name)
        assert _bits_equal(a[0], ref) and _bits_equal(a[1], ref), (k, n)
    assert np.float32(b.status(1).interface_level) == np.float32(o.status().if_level)
    b.close()


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_batch_above_8192_channels_runs_as_sub_batches(pkg, oracle, fmsig, dt):
    """8320 channels = a shell over two sub-batches (4224 + 4096): every sub-batch starts at its own row of the
    integer input (row offsets in bytes of the call's format)."""
    _run_stations(pkg, oracle, fmsig, dt, 2.4e6, 11, 8320, [N, 30001, N])


# ---------------------------------------------------------------------------------------------------------------
# captures

def _capture_rows(fmsig, fs, G, nblk, dt):
    """G captures of one stereo + RDS station each at -200 kHz, block by block, quantised"""
    st = [fmsig.default_params(fs, f_offset=-200e3, amp=0.3, noise_sigma=0.004, seed=300 + g, pi=0x7100 + g,
                               ps="CAP%d" % g) for g in range(G)]
    return [[_quant(fmsig.generate_f32(st[g], j * N, N), dt) for g in range(G)] for j in range(nblk)]


@pytest.mark.parametrize("fs,D,T,mode", [(1.0e6, 4, 10, 1), (2.4e6, 11, 24, 2)], ids=["k_if_fir", "k_if_fir_mt3"])
def test_captures_maps_and_switch_s16(pkg, oracle, fmsig, fs, D, T, mode):
    """4 captures x 8 stations (x 256 in the headline geometry with overlapped calls: the map form of k_if_fir_mt3)
    of S16 input: set_channels_per_capture, the same as an explicit map, a shuffled map, and a switch of channels to
    other captures at a call boundary -- against oracle decoders fed the spliced converted stream."""
    import torch
    dt, G, nblk, sw_at = np.int16, 4, 4, 2
    k = 8 if mode == 1 else 256
    C = G * k
    rows = _capture_rows(fmsig, fs, G, nblk, dt)
    step = fs / T
    tuned = int(round(200e3 / step))  # f(shift) = -shift fs / T = -200 kHz
    shifts = np.array([(tuned, tuned - 1, 0, tuned + 1)[c % 4] for c in range(C)], np.int32)
    st = torch.cuda.current_stream().cuda_stream

    def run(shifts, setup, switch=None):
        b = pkg.Batch(pkg.make_params(fs, 0.0, 48000.0, 15000.0, D, table_size=T), C, tuning_shifts=shifts,
                      record_callbacks=False)
        b.set_concurrency(mode)
        setup(b)
        a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
        keep, outs, nfs = [], [], []
        for j in range(nblk):
            if switch and j == sw_at:
                b.switch_captures(*switch)
            d_iq = torch.from_numpy(np.stack(rows[j])).cuda()
            d_out = torch.zeros((C, a_stride), dtype=torch.float32, device="cuda")
            keep.append(d_iq)
            outs.append(d_out)
            nfs.append(b.process_device(d_iq.data_ptr(), N, N, d_out.data_ptr(), a_stride, st, fmt=pkg.FMD_IQ_S16))
        b.wait(stream=st)
        torch.cuda.synchronize()
        audio = [outs[j][:, :nfs[j]].cpu().numpy() for j in range(nblk)]
        levels = [np.float32(b.status(c).interface_level) for c in range(C)]
        b.close()
        return audio, levels

    def splice(shift, seq):
        o = oracle.OracleDecoder(fs, 0.0, 48000.0, 15000.0, D, table_size=T, tuning_shift=int(shift))
        return o, [o.process_stream(_to_f32(rows[j][g])) for j, g in enumerate(seq)]

    cmap = np.arange(C) // k
    ref = run(shifts, lambda b: b.set_channels_per_capture(k))
    for c in (0, 1, k + 2, C - 1):
        o, out = splice(shifts[c], [c // k] * nblk)
        for j in range(nblk):
            assert _bits_equal(ref[0][j][c], out[j]), (c, j)
        assert ref[1][c] == np.float32(o.status().if_level), c
    got = run(shifts, lambda b: b.set_capture_map(cmap, G))
    for j in range(nblk):
        assert _bits_equal(got[0][j], ref[0][j]), j
    assert got[1] == ref[1]
    perm = np.random.default_rng(7).permutation(C)  # shuffled channel c plays contiguous channel perm[c]
    sh = run(shifts[perm], lambda b: b.set_capture_map(cmap[perm], G))
    for j in range(nblk):
        assert _bits_equal(sh[0][j], ref[0][j][perm]), j
    assert sh[1] == [ref[1][p] for p in perm]
    # a switch at the boundary in front of call sw_at: channels 0 and C - 1 trade captures, channel k + 2 moves on
    moved = {0: G - 1, C - 1: 0, k + 2: 2}
    sw = run(shifts, lambda b: b.set_capture_map(cmap, G),
             switch=(np.array(list(moved), np.uint32), np.array(list(moved.values()), np.uint32)))
    for c, g_new in moved.items():
        o, out = splice(shifts[c], [c // k] * sw_at + [g_new] * (nblk - sw_at))
        for j in range(nblk):
            assert _bits_equal(sw[0][j][c], out[j]), (c, j)
        assert sw[1][c] == np.float32(o.status().if_level), c
    others = np.array([c for c in range(C) if c not in moved])
    for j in range(nblk):
        assert _bits_equal(sw[0][j][others], ref[0][j][others]), j


# ---------------------------------------------------------------------------------------------------------------
# the format belongs to the call

def test_format_per_call_with_calls_in_flight(pkg, oracle, fmsig):
    """One batch fed f32, s16, u8, s8, s16, ... in successive calls, calls in flight and consumed two calls late: one
    oracle decoder per channel fed the converted stream (the IF delay line behind the tuner is float)."""
    import torch
    fs, D, C, lag = 2.4e6, 11, 6, 2
    ps = [fmsig.channel_params(fs, c) for c in range(C)]
    refs = [oracle.OracleDecoder(fs, -0.15 * fs, 48000.0, 15000.0, D) for _ in range(C)]
    b = pkg.Batch(pkg.make_params(fs, -0.15 * fs, 48000.0, 15000.0, D), C, record_callbacks=False)
    b.set_concurrency(2)
    st = torch.cuda.current_stream().cuda_stream
    a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
    seq = [np.float32, np.int16, np.uint8, np.int8, np.int16, np.float32, np.int8, np.uint8, np.int16, np.int16]
    sizes = [N, 30001, N, 8193, N, 20001, N, N, 33333, N]
    conv, keep, outs, nfs, start = [], [], [], [], 0
    for k, (dt, n) in enumerate(zip(seq, sizes)):
        n_al = (n + 1) // 2 * 2
        x = np.zeros((C, 2 * n_al), dtype=dt)
        f = np.zeros((C, 2 * n), dtype=np.float32)
        for c in range(C):
            if dt == np.float32:
                x[c, :2 * n] = f[c] = fmsig.generate_f32(ps[c], start, n)
            elif dt == np.uint8:
                x[c, :2 * n] = fmsig.generate_u8(ps[c], start, n)
                f[c] = oracle.convert_u8(x[c, :2 * n])
            else:
                x[c, :2 * n] = _quant(fmsig.generate_f32(ps[c], start, n), dt)
                f[c] = _to_f32(x[c, :2 * n])
        start += n
        conv.append(f)
        d_iq = torch.from_numpy(x).cuda()
        d_out = torch.zeros((C, a_stride), dtype=torch.float32, device="cuda")
        keep.append(d_iq)
        outs.append(d_out)
        nfs.append(b.process_device(d_iq.data_ptr(), n_al, n, d_out.data_ptr(), a_stride, st, fmt=_fmt(pkg, dt)))
        if k >= lag:
            b.wait(stream=st, lag=lag)
    b.wait(stream=st)
    groups = b.collect_rds_array(cap=65536, stream=st)
    torch.cuda.synchronize()
    for k in range(len(seq)):
        a = outs[k][:, :nfs[k]].cpu().numpy()
        for c in range(C):
            assert _bits_equal(a[c], refs[c].process_stream(conv[k][c])), (k, c)
    for c in range(C):
        mine = sorted((int(k), tuple(int(v) for v in bl)) for ch, k, bl in
                      zip(groups["channel"], groups["call_index"], groups["blocks"]) if ch == c)
        assert mine == sorted((k, tuple(bl)) for k, bl in refs[c].rds_groups()), c
        assert np.float32(refs[c].status().if_level) == np.float32(b.status(c).interface_level), c
    b.close()


def test_format_per_call_host_entry(pkg, oracle, fmsig):
    """The same through the host-buffer entry point (staging rows sized by the call's format)."""
    fs, D, C = 2.4e6, 11, 3
    ps = [fmsig.channel_params(fs, c) for c in range(C)]
    refs = [oracle.OracleDecoder(fs, -0.15 * fs, 48000.0, 15000.0, D) for _ in range(C)]
    b = pkg.Batch(pkg.make_params(fs, -0.15 * fs, 48000.0, 15000.0, D), C)
    start = 0
    for k, (dt, n) in enumerate([(np.int8, 8192), (np.int16, N), (np.float32, 20001), (np.int16, 33333),
                                 (np.uint8, N), (np.int8, N)]):
        f = np.stack([fmsig.generate_f32(ps[c], start, n) for c in range(C)])
        if dt == np.uint8:
            x = np.stack([fmsig.generate_u8(ps[c], start, n) for c in range(C)])
            f = np.stack([oracle.convert_u8(x[c]) for c in range(C)])
        elif dt != np.float32:
            x = _quant(f, dt)
            f = _to_f32(x)
        else:
            x = f
        start += n
        a = b.process_host_fmt(x)
        for c in range(C):
            assert _bits_equal(a[c], refs[c].process_stream(f[c])), (k, c)
    b.close()


# ---------------------------------------------------------------------------------------------------------------
# the old entry points are the new ones

@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_old_entry_points_equal_fmt(pkg, fmsig, u8):
    import torch
    fs, D, C, NB = 2.4e6, 11, 1024, 20  # (20 calls: RDS groups arrive)
    gen = fmsig.DeviceGenerator([fmsig.channel_params(fs, c % 8) for c in range(C)], "cuda")
    st = torch.cuda.current_stream().cuda_stream
    res = []
    for new in (False, True):
        b = pkg.Batch(pkg.make_params(fs, -0.15 * fs, 48000.0, 15000.0, D), C, record_callbacks=False)
        b.set_concurrency(2)
        a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
        outs, keep, nfs = [], [], []
        for k in range(NB):
            t = torch.empty((C, N, 2), dtype=torch.uint8 if u8 else torch.float32, device="cuda")
            gen.generate(t, k * N, N)
            d_out = torch.zeros((C, a_stride), dtype=torch.float32, device="cuda")
            keep.append(t)
            outs.append(d_out)
            if new:
                nfs.append(b.process_device(t.data_ptr(), N, N, d_out.data_ptr(), a_stride, st,
                                            fmt=pkg.FMD_IQ_U8 if u8 else pkg.FMD_IQ_F32))
            else:
                nfs.append(b.process_device(t.data_ptr(), N, N, d_out.data_ptr(), a_stride, st, u8=u8))
        b.wait(stream=st)
        g = b.collect_rds_array(cap=16 * C, stream=st)
        torch.cuda.synchronize()
        res.append(([outs[k][:, :nfs[k]].cpu().numpy() for k in range(NB)], g))
        b.close()
    for k in range(NB):
        assert _bits_equal(res[0][0][k], res[1][0][k]), k
    assert len(res[0][1]) > 0 and np.array_equal(np.sort(res[0][1], order=["channel", "call_index"]),
                                                 np.sort(res[1][1], order=["channel", "call_index"]))
    # host entry points
    x = fmsig.generate_u8(fmsig.default_params(fs), 0, N)
    f = fmsig.u8_to_f32(x)
    b0 = pkg.Batch(pkg.make_params(fs, -0.15 * fs, 48000.0, 15000.0, D), 1)
    b1 = pkg.Batch(pkg.make_params(fs, -0.15 * fs, 48000.0, 15000.0, D), 1)
    old = b0.process_host_u8(x, shared=True) if u8 else b0.process_host(f.view(np.complex64), shared=True)
    assert _bits_equal(old, b1.process_host_fmt(x if u8 else f, shared=True))
    b0.close()
    b1.close()


# ---------------------------------------------------------------------------------------------------------------
# alignment

@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_device_entry_rejects_misaligned_stride_and_pointer(pkg, dt):
    import torch
    fs, D = 2.4e6, 11
    b = pkg.Batch(pkg.make_params(fs, -0.15 * fs, 48000.0, 15000.0, D), 2)
    esz = pkg.IQ_BYTES[_fmt(pkg, dt)]
    iq = torch.zeros(2 * N * esz + 64, dtype=torch.uint8, device="cuda")
    audio = torch.zeros(2 * b.max_audio_floats(N), dtype=torch.float32, device="cuda")
    a_stride = b.max_audio_floats(N)
    with pytest.raises(pkg.FmdError, match="two IQ samples"):
        b.process_device(iq.data_ptr(), N + 1, N, audio.data_ptr(), a_stride, fmt=_fmt(pkg, dt))
    with pytest.raises(pkg.FmdError, match="two IQ samples"):
        b.process_device(iq.data_ptr() + esz, N, N, audio.data_ptr(), a_stride, fmt=_fmt(pkg, dt))
    b.process_device(iq.data_ptr(), N, N, audio.data_ptr(), a_stride, fmt=_fmt(pkg, dt))  # aligned: taken
    torch.cuda.synchronize()
    b.close()


# ---------------------------------------------------------------------------------------------------------------
# scan

@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_scan_gives_the_bits_of_the_float_scan(pkg, fmsig, dt):
    """S8 / S16 accumulate (device and host entry): PSD, slot powers, floor and candidate list of the float scan of
    the converted captures; the row a capture sits in and the capture count do not matter."""
    import torch
    scanmod = import_module(pkg.__name__ + ".scan")
    FS, G, n = 2.4e6, 3, 40000
    q = np.stack([_quant(fmsig.generate_f32(fmsig.default_params(FS, f_offset=(g - 1) * 400e3, seed=7 + g), 0, n), dt)
                  for g in range(G)])
    f32 = _to_f32(q)

    def same(ra, rb, what):
        for key in ("psd", "slot_db", "floor_db"):
            rows = [g for g in range(len(ra[key])) if not _bits_equal(ra[key][g], rb[key][g])]
            assert not rows, (what, key, rows, [float(ra["psd"][g].sum() / rb["psd"][g].sum()) for g in rows])
        assert ra["candidates"] == rb["candidates"] and np.array_equal(ra["counts"], rb["counts"]), what

    for nfft in (256, 1024, 4096):
        fl = scanmod.Scan(FS, G, nfft=nfft)
        fl.accumulate_host(f32)
        rf = fl.result()
        assert sum(len(c) for c in rf["candidates"]) >= G  # the stations are found: not a scan of nothing
        host = scanmod.Scan(FS, G, nfft=nfft)
        host.accumulate_host(q)  # by dtype: fmd_scan_accumulate_host_fmt
        same(host.result(), rf, (nfft, "host"))
        # the device entry point with a row stride longer than a capture, on a stream of its own
        d = torch.zeros((G, 2 * (n + 64)), dtype=torch.from_numpy(q).dtype, device="cuda")
        d[:, :2 * n] = torch.from_numpy(q).cuda()
        torch.cuda.synchronize()
        dev = scanmod.Scan(FS, G, nfft=nfft)
        s = torch.cuda.Stream()
        dev.accumulate_device(d.data_ptr(), n + 64, n, stream=s.cuda_stream, fmt=_fmt(pkg, dt))
        s.synchronize()
        same(dev.result(), rf, (nfft, "device"))
        # rows in another order, and every capture alone
        perm = [2, 0, 1]
        pr = scanmod.Scan(FS, G, nfft=nfft)
        pr.accumulate_host(q[perm])
        rp = pr.result()
        assert np.array_equal(rp["psd"].view(np.uint32), rf["psd"][perm].view(np.uint32))
        assert rp["candidates"] == [rf["candidates"][g] for g in perm]
        for g in range(G):
            one = scanmod.Scan(FS, 1, nfft=nfft)
            one.accumulate_host(q[g])
            r1 = one.result()
            assert np.array_equal(r1["psd"][0].view(np.uint32), rf["psd"][g].view(np.uint32)), (nfft, g)
            assert r1["candidates"][0] == rf["candidates"][g]
            one.close()
        for x in (fl, host, dev, pr):
            x.close()
    # many captures: the one-workgroup-per-capture form
    Gm = 520
    big = np.tile(q, (Gm // G + 1, 1))[:Gm]
    a = scanmod.Scan(FS, Gm)
    a.accumulate_host(big)
    bf = scanmod.Scan(FS, Gm)
    bf.accumulate_host(_to_f32(big))
    same(a.result(), bf.result(), "520 captures")
    a.close()
    bf.close()
    with pytest.raises(pkg.FmdError, match="two IQ samples"):
        s = scanmod.Scan(FS, 1)
        try:
            s.accumulate_device(d.data_ptr() + pkg.IQ_BYTES[_fmt(pkg, dt)], n, n, fmt=_fmt(pkg, dt))
        finally:
            s.close()


def test_scan_stations_takes_integer_captures(pkg, fmsig):
    """scan_stations passes the captures' dtype through to the scan and to its confirming batch: the stations of
    S16 captures are those of the converted float captures, field for field."""
    scanmod = import_module(pkg.__name__ + ".scan")
    FS, G = 2.4e6, 2
    st = [[fmsig.default_params(FS, f_offset=f0, amp=0.2, noise_sigma=0.004, seed=90 + 7 * g + i, pi=0x6000 + 16 * g + i,
                                ps="ST%d%d    " % (g, i)) for i, f0 in enumerate((-500e3, 300e3))] for g in range(G)]

    def capture(call, g):
        x = np.zeros(2 * N, np.float32)
        for p in st[g]:
            x += fmsig.generate_f32(p, call * N, N)
        return _quant(x, np.int16)

    cache = {}

    def src_q(call):
        if call not in cache:
            cache[call] = np.stack([capture(call, g) for g in range(G)])
        return cache[call]

    got = scanmod.scan_stations(src_q, G, FS, scan_calls=2, confirm_calls=30)
    want = scanmod.scan_stations(lambda call: _to_f32(src_q(call)).view(np.complex64), G, FS, scan_calls=2,
                                 confirm_calls=30)
    assert got == want
    assert [len(x) for x in got] == [2, 2]
    assert all(s["stereo"] and s["pi"] is not None for x in got for s in x)


# ---------------------------------------------------------------------------------------------------------------
# receiver

def test_receiver_blocks_carry_their_format(pkg, fmsig):
    """Blocks written as s16, f32, u8, s8 in turn produce the packets (stream id, PTS, duration, payload bytes) and
    the signal status of a receiver fed the converted floats."""
    fs, D, nblk = 2.4e6, 11, 36
    p = fmsig.default_params(fs, noise_sigma=0.01, seed=3, pi=0xFDFE, ps="FORMATS ")
    blocks = []
    for k in range(nblk):
        dt = (np.int16, np.float32, np.uint8, np.int8)[k % 4]
        if dt == np.uint8:
            x = fmsig.generate_u8(p, k * N, N)
            f = fmsig.u8_to_f32(x)
        elif dt == np.float32:
            x = f = fmsig.generate_f32(p, k * N, N)
        else:
            x = _quant(fmsig.generate_f32(p, k * N, N), dt)
            f = _to_f32(x)
        blocks.append((x, f))

    def session(rx, which, write):
        packets, status, written = [], [], 0
        while True:
            while written < nblk and rx.queued_samples() < 2 * N:
                write(rx, blocks[written][which])
                written += 1
            if written == nblk:
                rx.end()
            pkt = rx.demux_read()
            if pkt is None:
                break
            packets.append(pkt)
            if pkt[0] == 1:
                status.append((rx.signal_status(), rx.pvr_signal_status()))
        return packets, status

    ra = pkg.Receiver(fs, -0.15 * fs, D)
    rb = pkg.Receiver(fs, -0.15 * fs, D)
    pa, sa = session(ra, 0, lambda rx, x: rx.write(x))
    pb, sb = session(rb, 1, lambda rx, x: rx.write_iq(x))
    assert len(pa) == len(pb) and len(pa) >= nblk
    for a, b in zip(pa, pb):
        assert a == b
    assert sum(k[0] == 2 for k in pa) >= 2  # RDS packets: not silence
    for (a3, apvr), (b3, bpvr) in zip(sa, sb):
        assert np.float32(a3[0]).view(np.uint32) == np.float32(b3[0]).view(np.uint32)
        assert np.float32(a3[1]).view(np.uint32) == np.float32(b3[1]).view(np.uint32)
        assert a3[2] == b3[2] and apvr == bpvr
    ra.close()
    rb.close()
