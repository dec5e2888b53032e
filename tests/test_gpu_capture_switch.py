"""Capture maps and capture switches (fmd_batch_set_capture_map / fmd_batch_switch_captures /
fmd_batch_retune_channels_to, include/fmd.h), bit for bit.

A switched channel must decode like an oracle decoder fed the spliced stream: the old capture's blocks before the
boundary and the new capture's after it, with all its state carried over.  Channels that were not switched must equal
the same batch run without the switch.  Oracle decoders run only for the channels checked."""
import itertools
import math

import numpy as np
import pytest
import torch

from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

N = 65536
FS, D, T = 1.0e6, 4, 10  # tuner table of 10 entries: a shift step is 100 kHz
HFS, HD, HT = 2.4e6, 11, 24  # the headline geometry (its IF FIR is k_if_fir_mt3 in concurrency mode 2)


@pytest.fixture(scope="module")
def pkg_fixture():
    return load_package()


def _params(pkg, fs=FS, d=D, t=T):
    return pkg.make_params(fs, 0.0, 48000.0, 15000.0, d, table_size=t)


def _oracle(oracle, shift, fs=FS, d=D, t=T):
    return oracle.OracleDecoder(fs, 0.0, 48000.0, 15000.0, d, table_size=t, tuning_shift=int(shift))


def _bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _status_tuple(s):
    return (bool(s.stereo_detected), np.float32(s.tuning_offset), np.float32(s.interface_level),
            np.float32(s.pilot_level))


def _oracle_status(s):
    return (bool(s.stereo), np.float32(s.tuning_offset), np.float32(s.if_level), np.float32(s.pilot_level))


def _station(fmsig, g, fs=FS, f_offset=None):
    """capture g's station: stereo + RDS (its own PI and PS) for even g, mono for odd g"""
    f = f_offset if f_offset is not None else (-200e3 if g % 2 == 0 else 100e3)
    if g % 2 == 0:
        return fmsig.default_params(fs, f_offset=f, amp=0.3, noise_sigma=0.004, seed=300 + g, pi=0x7100 + g,
                                    ps="CAP%d" % g)
    return fmsig.mono_params(fs, f_offset=f, amp=0.2, noise_sigma=0.004, seed=300 + g)


class Captures:
    """G captures of one station each, block by block (float32 interleaved or RTL-SDR bytes)"""

    def __init__(self, fmsig, G, u8=False, fs=FS):
        self.st = [_station(fmsig, g, fs) for g in range(G)]
        self.fmsig, self.u8, self.cache = fmsig, u8, {}

    def row(self, g, j):
        if (g, j) not in self.cache:
            gen = self.fmsig.generate_u8 if self.u8 else self.fmsig.generate_f32
            self.cache[(g, j)] = gen(self.st[g], j * N, N)
        return self.cache[(g, j)]

    def block(self, j):
        return np.stack([self.row(g, j) for g in range(len(self.st))])


def _process(b, caps, j):
    x = caps.block(j)
    return b.process_host_u8(x) if caps.u8 else b.process_host(x.view(np.complex64))


def _oracle_splice(oracle, shift, caps, seq, resets=(), zeros_before=0, fs=FS, d=D, t=T):
    """an oracle decoder fed capture seq[j] in call j (zeros before call `zeros_before`), reset in front of the calls
    in `resets`; returns (decoder, audio per call, taps of every call)"""
    o = _oracle(oracle, shift, fs, d, t)
    out, taps = [], []
    for j, g in enumerate(seq):
        if j in resets:
            o.reset()
        if j < zeros_before:
            out.append(o.process_stream(np.zeros(2 * N, np.float32)))
        elif caps.u8:
            out.append(o.process_stream_u8(caps.row(g, j)))
        else:
            out.append(o.process_stream(caps.row(g, j)))
        taps.append(o.taps()["demod"].copy())
    return o, out, taps


# ---------------------------------------------------------------------------------------------------------------
# 1, 2: maps against the contiguous rule

@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_contiguous_and_shuffled_maps_small(pkg_fixture, oracle, fmsig, u8):
    """16 channels over 4 captures (k_if_fir forms): an explicit contiguous map gives the bits of
    set_channels_per_capture(4); a shuffled map gives every channel the bits of its counterpart (same capture, same
    shift), with the capture-ordered walk and without; two channels also equal the oracle."""
    pkg = pkg_fixture
    G, k, nblk = 4, 4, 4
    C = G * k
    caps = Captures(fmsig, G, u8)
    shifts = np.array([2, -1, 0, 3] * G, np.int32)  # 2: the stereo station of the even captures, -1: the mono one

    def run(shifts, setup):
        b = pkg.Batch(_params(pkg), C, tuning_shifts=shifts)
        setup(b)
        audio = [_process(b, caps, j) for j in range(nblk)]
        st = [_status_tuple(b.status(c)) for c in range(C)]
        fr = [b.sink.frames.get(c, []) for c in range(C)]
        b.close()
        return audio, st, fr

    ref = run(shifts, lambda b: b.set_channels_per_capture(k))
    cmap = np.arange(C) // k
    got = run(shifts, lambda b: b.set_capture_map(cmap, G))
    for j in range(nblk):
        assert _bits(got[0][j], ref[0][j]), j
    assert got[1] == ref[1] and got[2] == ref[2]
    perm = np.random.default_rng(7).permutation(C)  # shuffled channel c plays contiguous channel perm[c]
    for walk in (1, 0):
        def setup(b, walk=walk):
            b.set_capture_map(cmap[perm], G)
            b.debug_capture_walk(walk)
        sh = run(shifts[perm], setup)
        for j in range(nblk):
            assert _bits(sh[0][j], ref[0][j][perm]), (walk, j)
        assert sh[1] == [ref[1][p] for p in perm] and sh[2] == [ref[2][p] for p in perm], walk
    for c in (0, 6):  # contiguous channel 0: capture 0's stereo station; 6: capture 1, shift 0
        _, out, _ = _oracle_splice(oracle, shifts[c], caps, [c // k] * nblk)
        for j in range(nblk):
            assert _bits(ref[0][j][c], out[j]), (c, j)


def test_contiguous_and_shuffled_maps_headline(pkg_fixture, fmsig):
    """1024 channels over 8 captures at 2.4 MS/s in concurrency mode 2 (the headline IF FIR form, k_if_fir_mt3):
    the explicit contiguous map and a shuffled map give every channel its counterpart's bits, groups (with their call
    index) and status records."""
    pkg = pkg_fixture
    G, C, nblk = 8, 1024, 12  # (12 calls: time for RDS to sync on the stereo captures)
    k = C // G
    rows = [[torch.from_numpy(fmsig.generate_f32(_station(fmsig, g, HFS, f_offset=(-300e3 + 100e3 * g)), j * N, N))
             for g in range(G)] for j in range(nblk)]
    blocks = [torch.stack(r).cuda() for r in rows]
    shifts = np.resize(np.array([3, 2, 1, 0, -1, -2, -3, -4], np.int32), C)
    perm = np.random.default_rng(11).permutation(C)

    def run(shifts, setup):
        b = pkg.Batch(_params(pkg, HFS, HD, HT), C, tuning_shifts=shifts, record_callbacks=False)
        setup(b)
        b.set_concurrency(2)
        a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
        audio = torch.zeros((nblk, C, a_stride), dtype=torch.float32, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        nf = [b.process_device(blocks[j].data_ptr(), N, N, audio[j].data_ptr(), a_stride, s) for j in range(nblk)]
        b.wait(stream=s)
        g = b.collect_rds_array()
        torch.cuda.synchronize()
        st = [_status_tuple(b.status(c)) for c in range(C)]
        b.close()
        return [audio[j][:, :nf[j]].cpu().numpy() for j in range(nblk)], g, st

    ref = run(shifts, lambda b: b.set_channels_per_capture(k))
    got = run(shifts, lambda b: b.set_capture_map(np.arange(C) // k, G))
    sh = run(shifts[perm], lambda b: b.set_capture_map((np.arange(C) // k)[perm], G))
    inv = np.argsort(perm)
    for j in range(nblk):
        assert _bits(got[0][j], ref[0][j]), j
        assert _bits(sh[0][j], ref[0][j][perm]), j
    key = lambda g: sorted((int(c), int(k_), tuple(int(x) for x in bl)) for c, k_, bl in g)
    assert len(ref[1]) > 0
    assert key(got[1]) == key(ref[1])
    renamed = [(int(perm[c]), int(k_), tuple(int(x) for x in bl)) for c, k_, bl in sh[1]]
    assert sorted(renamed) == key(ref[1])
    assert got[2] == ref[2]
    assert [sh[2][inv[c]] for c in range(C)] == ref[2]


# ---------------------------------------------------------------------------------------------------------------
# 3, 9: a switch in the default mode, against the oracle, with teeth

def test_switch_in_default_mode(pkg_fixture, oracle, fmsig):
    """16 channels over 4 captures; before call K channel 2 (stereo station of capture 0) moves to capture 2, channel
    5 (capture 1, shift -1: the mono station) to capture 3, channel 12 (capture 3, shift 2: nothing) to capture 0.
    The demod tap of call K mixes both captures; audio, getters, UECP frames and name follow the oracle fed the
    splice; every other channel equals the run without the switch.  The oracle fed the splice one call early or
    late does NOT agree (the boundary is seen)."""
    pkg = pkg_fixture
    G, k, nblk, K = 4, 4, 8, 4
    C = G * k
    caps = Captures(fmsig, G)
    shifts = np.array([0, -1, 2, 1] * G, np.int32)
    shifts[12] = 2
    moves = {2: 2, 5: 3, 12: 0}

    def run(switch):
        b = pkg.Batch(_params(pkg), C, tuning_shifts=shifts)
        b.set_capture_map(np.arange(C) // k, G)
        b.enable_taps(True)
        audio, frames_before, demod = [], None, {}
        for j in range(nblk):
            if switch and j == K:
                frames_before = {c: len(b.sink.frames.get(c, [])) for c in moves}
                b.switch_captures(list(moves), list(moves.values()))
                m, n = b.capture_map()
                assert n == G and all(m[c] == g for c, g in moves.items())
            audio.append(_process(b, caps, j))
            if j == K:
                demod = {c: b.tap("demod", c) for c in moves}
        return b, audio, frames_before, demod

    b, audio, fb, demod = run(True)
    ref, audio_ref, _, _ = run(False)
    for j in range(nblk):
        for c in range(C):
            if c not in moves or j < K:
                assert _bits(audio[j][c], audio_ref[j][c]), (j, c)
    for c, g in moves.items():
        seq = [c // k] * K + [g] * (nblk - K)
        o, out, taps = _oracle_splice(oracle, shifts[c], caps, seq)
        assert _bits(demod[c].view(np.float32), taps[K].view(np.float32)), c
        for j in range(nblk):
            assert _bits(audio[j][c], out[j]), (c, j)
        assert _status_tuple(b.status(c)) == _oracle_status(o.status()), c
        assert b.status_call_index(c) == nblk
        assert b.sink.frames.get(c, []) == o.uecp_frames(), c  # one group decoder across the switch
        if o.channel_name().strip():
            assert b.sink.names.get(c) == o.channel_name(), c
        # teeth: the splice one call early / late gives other bits somewhere from K - 1 on
        for shift_by in (-1, 1):
            seq2 = [c // k] * (K + shift_by) + [g] * (nblk - K - shift_by)
            _, out2, _ = _oracle_splice(oracle, shifts[c], caps, seq2)
            assert not all(_bits(audio[j][c], out2[j]) for j in range(nblk)), (c, shift_by)
    assert len(b.sink.frames.get(2, [])) > fb[2]  # channel 2 kept receiving groups across the switch
    for c in range(C):
        if c not in moves:
            assert _status_tuple(b.status(c)) == _status_tuple(ref.status(c)), c
            assert b.sink.frames.get(c, []) == ref.sink.frames.get(c, []), c
    b.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------
# 4: calls in flight, mode 0 and profiling level 2

@pytest.mark.parametrize("mode", ["c2-lag1", "c2-lag2", "c2-lag3", "mode0", "prof2"])
def test_switch_with_calls_in_flight(pkg_fixture, oracle, fmsig, mode):
    """Device calls; concurrency 2 with outputs consumed `lag` calls late (the switch is made while earlier calls
    run: they keep the old capture), concurrency 0 and profiling level 2 (the IF stage on the caller's stream).
    Groups with their call index too."""
    pkg = pkg_fixture
    G, k, nblk, K = 4, 64, 7, 3
    C = G * k
    caps = Captures(fmsig, G)
    blocks = [torch.from_numpy(caps.block(j)).cuda() for j in range(nblk)]
    shifts = np.resize(np.array([2, -1, 0, 1], np.int32), C)
    moves = {0: 2, 70: 0, 255: 1}
    lag = int(mode[-1]) if mode.startswith("c2") else 0

    def run(switch):
        b = pkg.Batch(_params(pkg), C, tuning_shifts=shifts, record_callbacks=False)
        b.set_capture_map(np.arange(C) // k, G)
        if mode.startswith("c2"):
            b.set_concurrency(2)
        elif mode == "mode0":
            b.set_concurrency(0)
        else:
            b.set_profiling(2)
        a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
        audio = [torch.zeros((C, a_stride), dtype=torch.float32, device="cuda") for _ in range(nblk)]
        s = torch.cuda.current_stream().cuda_stream
        nf, groups = [], []
        for j in range(nblk):
            if switch and j == K:
                b.switch_captures(list(moves), list(moves.values()))
            nf.append(b.process_device(blocks[j].data_ptr(), N, N, audio[j].data_ptr(), a_stride, s))
            if lag and j >= lag:
                b.wait(stream=s, lag=lag)
        b.wait(stream=s)
        groups = b.collect_rds_array()
        torch.cuda.synchronize()
        st = {c: _status_tuple(b.status(c)) for c in moves}
        b.close()
        return [audio[j][:, :nf[j]].cpu().numpy() for j in range(nblk)], groups, st

    got, g_got, st = run(True)
    ref, g_ref, _ = run(False)
    for j in range(nblk):
        keep = [c for c in range(C) if c not in moves or j < K]
        assert np.array_equal(got[j][keep].view(np.uint32), ref[j][keep].view(np.uint32)), j
    for c, g in moves.items():
        o, out, _ = _oracle_splice(oracle, shifts[c], caps, [c // k] * K + [g] * (nblk - K))
        for j in range(nblk):
            assert _bits(got[j][c], out[j]), (mode, c, j)
        assert st[c] == _oracle_status(o.status()), c
    others = lambda g: sorted((int(c), int(kk), tuple(int(x) for x in bl)) for c, kk, bl in g if int(c) not in moves)
    assert others(g_got) == others(g_ref)
    before = lambda g, c: sorted((int(kk), tuple(int(x) for x in bl)) for cc, kk, bl in g if int(cc) == c and kk <= K)
    for c in moves:  # groups of the calls before the switch are the old capture's
        assert before(g_got, c) == before(g_ref, c), c


# ---------------------------------------------------------------------------------------------------------------
# 5, 7: several edits of one channel before one call; retune to a capture

def test_last_switch_wins_and_edits_apply_in_order(pkg_fixture, oracle, fmsig):
    """Three switches of one channel before one call: the last capture counts.  Switch, reset and retune-to of one
    channel in all six orders before one call: applied in the order made (a retune replaces the state a reset in
    front of it cleared; the last capture wins)."""
    pkg = pkg_fixture
    G, nblk, K = 4, 5, 2
    caps = Captures(fmsig, G)
    orders = list(itertools.permutations(["switch", "reset", "retune"]))
    C = 4 + len(orders)
    shifts = np.array([2] * C, np.int32)
    b = pkg.Batch(_params(pkg), C, tuning_shifts=shifts)
    b.enable_retune()
    cmap = np.array([0] * C, np.uint32)
    b.set_capture_map(cmap, G)
    audio = []
    for j in range(nblk):
        if j == K:
            for g in (1, 3, 2):
                b.switch_captures([1], [g])
            for i, order in enumerate(orders):
                c = 4 + i
                for e in order:
                    if e == "switch":
                        b.switch_captures([c], [1])
                    elif e == "reset":
                        b.reset_channels([c])
                    else:
                        b.retune([c], [-1], captures=[3])
        audio.append(_process(b, caps, j))
    _, out, _ = _oracle_splice(oracle, 2, caps, [0] * K + [2] * (nblk - K))
    for j in range(nblk):
        assert _bits(audio[j][1], out[j]), j
    for i, order in enumerate(orders):
        c = 4 + i
        g = 1 if order.index("switch") > order.index("retune") else 3
        resets = (K,) if order.index("reset") > order.index("retune") else ()
        o, out, _ = _oracle_splice(oracle, -1, caps, [0] * K + [g] * (nblk - K), resets=resets, zeros_before=K)
        for j in range(K, nblk):
            assert _bits(audio[j][c], out[j]), (order, j)
        assert _status_tuple(b.status(c)) == _oracle_status(o.status()), order
    b.close()


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_retune_to_a_capture(pkg_fixture, oracle, fmsig, u8):
    """retune(channels, shifts, captures): like an oracle created with the new shift that received zeros, then the
    new capture's blocks; the other channels do not notice."""
    pkg = pkg_fixture
    G, nblk, K = 4, 6, 3
    caps = Captures(fmsig, G, u8)
    C = 8
    shifts = np.array([-1, 2, 0, 1, 2, -1, 0, 1], np.int32)
    cmap = np.arange(C) % G

    def run(edit):
        b = pkg.Batch(_params(pkg), C, tuning_shifts=shifts)
        b.enable_retune()
        b.set_capture_map(cmap, G)
        audio = []
        for j in range(nblk):
            if edit and j == K:
                b.retune([3, 6], [2, -1], captures=[2, 1])
            audio.append(_process(b, caps, j))
        return b, audio

    b, audio = run(True)
    ref, audio_ref = run(False)
    for c, s, g in ((3, 2, 2), (6, -1, 1)):
        o, out, _ = _oracle_splice(oracle, s, caps, [g] * nblk, zeros_before=K)
        for j in range(K, nblk):
            assert _bits(audio[j][c], out[j]), (c, j)
        assert _status_tuple(b.status(c)) == _oracle_status(o.status()), c
        if o.channel_name().strip():
            assert b.sink.names.get(c) == o.channel_name(), c
    for j in range(nblk):
        for c in range(C):
            if c not in (3, 6) or j < K:
                assert _bits(audio[j][c], audio_ref[j][c]), (j, c)
    assert list(b.capture_map()[0]) == [0, 1, 2, 2, 0, 1, 1, 3]
    b.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------
# 6: sub-batches

def test_switch_across_sub_batches(pkg_fixture, oracle, fmsig):
    """16 384 channels run as two sub-batches of 8192; capture 1's channels lie on both sides of 8192 (refused by
    the channels-per-capture rule); switches cross the boundary both ways."""
    pkg = pkg_fixture
    G, nblk, K, C = 3, 5, 2, 16384
    caps = Captures(fmsig, G)
    blocks = [torch.from_numpy(caps.block(j)).cuda() for j in range(nblk)]
    cmap = np.where(np.arange(C) < 4096, 0, np.where(np.arange(C) < 12288, 1, 2)).astype(np.uint32)
    shifts = np.resize(np.array([2, -1, 0, 1], np.int32), C)
    b = pkg.Batch(_params(pkg), C, tuning_shifts=shifts, record_callbacks=False)
    b.set_capture_map(cmap, G)
    moves = {4: 1, 8190: 2, 8192: 0, 16380: 1}
    a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
    audio = torch.zeros((nblk, C, a_stride), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    nf = []
    for j in range(nblk):
        if j == K:
            b.switch_captures(list(moves), list(moves.values()))
        nf.append(b.process_device(blocks[j].data_ptr(), N, N, audio[j].data_ptr(), a_stride, s))
    b.wait(stream=s)
    torch.cuda.synchronize()
    got = [audio[j][:, :nf[j]].cpu().numpy() for j in range(nblk)]
    for c in list(moves) + [5000, 9000, 13000]:
        g_new = moves.get(c, int(cmap[c]))
        o, out, _ = _oracle_splice(oracle, shifts[c], caps, [int(cmap[c])] * K + [g_new] * (nblk - K))
        for j in range(nblk):
            assert _bits(got[j][c], out[j]), (c, j)
        assert _status_tuple(b.status(c)) == _oracle_status(o.status()), c
    for j in range(nblk):  # capture 1, same shift, in either sub-batch
        assert _bits(got[j][4100], got[j][12284]), j
    b.close()


# ---------------------------------------------------------------------------------------------------------------
# 8: the reference's own seek

SEEK_FS, SEEK_D, SEEK_T = 1.0e6, 4, 10
SEEK_SHIFT = -2  # every seek channel listens 200 kHz above its capture's LO
DWELL = math.ceil(1.25 * SEEK_FS / N)  # calls per seek step (ChannelSettings.cpp: a step every 1.25 s)
NCAP = 24  # the dongle's LO 100 kHz higher per capture
# the band, in 100 kHz steps above capture 0's listening frequency: stereo stations (with RDS) and mono ones
BAND = {1: "stereo", 3: "mono", 5: "stereo", 12: "stereo", 14: "mono", 21: "mono"}


class Band:
    """capture j: what a dongle with its LO at 100 kHz * j sees of BAND (stations within 400 kHz of the LO)"""

    def __init__(self, fmsig):
        self.fmsig, self.cache = fmsig, {}

    def row(self, j, call):
        if (j, call) not in self.cache:
            x = np.zeros(2 * N, np.float32)
            for pos, kind in BAND.items():
                f = (pos - j) * 100e3 + 200e3  # the station's offset from this capture's LO
                if abs(f) <= 400e3:
                    kw = dict(f_offset=f, noise_sigma=0.0, seed=500 + pos)
                    p = self.fmsig.default_params(SEEK_FS, amp=0.25, pi=0x7200 + pos, **kw) if kind == "stereo" \
                        else self.fmsig.mono_params(SEEK_FS, amp=0.25, **kw)
                    x += self.fmsig.generate_f32(p, call * N, N)
            x += self.fmsig.generate_f32(self.fmsig.mono_params(SEEK_FS, amp=0.0, noise_sigma=0.004, seed=900 + j),
                                         call * N, N)
            self.cache[(j, call)] = x
        return self.cache[(j, call)]


def _seek_step(cur, up):
    """ChannelSettings.cpp:101-116: one step up or down, wrapping over the band's ends"""
    return (cur + 1) % NCAP if up else (cur - 1) % NCAP


def test_seek_like_the_reference(pkg_fixture, oracle, fmsig):
    """Seek channels (different starts, both directions) in one batch: each reads a capture, and after every dwell of
    1.25 s in which it does not report stereo, switches to the next capture.  Each must visit the same captures, stop
    at the same one and report the same getters at every dwell's end as an oracle decoder fed the same spliced
    stream (the stop is decided from the getters: the pilot lock counter and everything else carry over)."""
    pkg = pkg_fixture
    band = Band(fmsig)
    starts = [(3, True), (13, False), (22, True), (7, False)]
    C = len(starts)
    b = pkg.Batch(_params(pkg, SEEK_FS, SEEK_D, SEEK_T), C, tuning_shifts=np.full(C, SEEK_SHIFT, np.int32),
                  record_callbacks=False)
    b.set_capture_map(np.array([s for s, _ in starts], np.uint32), NCAP)
    orc = [_oracle(oracle, SEEK_SHIFT, SEEK_FS, SEEK_D, SEEK_T) for _ in range(C)]
    cur_b = [s for s, _ in starts]
    cur_o = list(cur_b)
    done_b, done_o = [False] * C, [False] * C
    visits_b = [[s] for s, _ in starts]
    visits_o = [[s] for s, _ in starts]
    call = 0
    while not (all(done_b) and all(done_o)) and call < 8 * DWELL:
        x = np.zeros((NCAP, 2 * N), np.float32)  # rows no channel reads stay zeros
        for j in set(cur_b):
            x[j] = band.row(j, call)
        b.process_host(x.view(np.complex64))
        for c in range(C):
            orc[c].process_stream(band.row(cur_o[c], call))
        call += 1
        if call % DWELL:
            continue
        switch = {}
        for c, (_, up) in enumerate(starts):
            sb, so = _status_tuple(b.status(c)), _oracle_status(orc[c].status())
            assert sb == so, (c, call, visits_b[c])
            if not done_b[c]:
                if sb[0]:
                    done_b[c] = True
                else:
                    cur_b[c] = _seek_step(cur_b[c], up)
                    visits_b[c].append(cur_b[c])
                    switch[c] = cur_b[c]
            if not done_o[c]:
                if so[0]:
                    done_o[c] = True
                else:
                    cur_o[c] = _seek_step(cur_o[c], up)
                    visits_o[c].append(cur_o[c])
        if switch:
            b.switch_captures(list(switch), list(switch.values()))
    assert visits_b == visits_o
    assert all(done_b) and all(done_o), visits_b
    assert sum(len(v) > 1 for v in visits_b) >= 2, visits_b  # the seeks did move
    b.close()


# ---------------------------------------------------------------------------------------------------------------
# 10: errors

def test_capture_map_errors(pkg_fixture, fmsig):
    """Out-of-range channel or capture, a channel listed twice, n_captures == 0, a map naming a capture beyond it,
    retune-to without retuning enabled: FMD_ERR_ARG / FMD_ERR_STATE with a sentence; the batch stays usable."""
    pkg = pkg_fixture
    G, C = 4, 8
    caps = Captures(fmsig, G)
    b = pkg.Batch(_params(pkg), C, tuning_shifts=np.zeros(C, np.int32))
    with pytest.raises(pkg.FmdError, match="no captures"):
        b.set_capture_map(np.zeros(C, np.uint32), 0)
    with pytest.raises(pkg.FmdError, match="reads capture 4 of 4"):
        b.set_capture_map(np.array([0, 1, 2, 3, 4, 0, 0, 0], np.uint32), G)
    b.set_capture_map(np.arange(C) % G, G)
    with pytest.raises(pkg.FmdError, match="channel 8 out of range"):
        b.switch_captures([8], [0])
    with pytest.raises(pkg.FmdError, match="capture 4 out of range"):
        b.switch_captures([1], [4])
    with pytest.raises(pkg.FmdError, match="twice"):
        b.switch_captures([1, 1], [0, 2])
    with pytest.raises(pkg.FmdError, match="not enabled"):
        b.retune([1], [2], captures=[1])
    assert pkg.lib().fmd_batch_switch_captures(b._h, None, None, 0) == -1
    assert b"null" in pkg.lib().fmd_last_error()
    assert list(b.capture_map()[0]) == list(np.arange(C) % G)
    b.switch_captures([], [])  # nothing to do
    a = _process(b, caps, 0)
    assert a.shape[0] == C and np.isfinite(a).all()
    # without a map, a switch starts from the channels-per-capture rule
    b.set_channels_per_capture(2)
    assert b.capture_map()[1] == 4
    b.switch_captures([7], [0])
    m, n = b.capture_map()
    assert n == 4 and list(m) == [0, 0, 1, 1, 2, 2, 3, 0]
    _process(b, caps, 1)
    b.set_capture_map(None, 0)
    assert b.capture_map()[1] == C
    b.close()
