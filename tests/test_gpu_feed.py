"""The mono feed at sample_rate_pcm / 2 or / 3 beside the audio (FMD_FEED_*, include/fmd.h): the
feed forms of the audio tail, k_feed_out / k_feed_out_sel and the history roll, through every entry point.

No tolerance anywhere: every delivered sample equals tests/feed_spec.py -- the definition restated in numpy float32 --
applied to the CPU oracle's audio of the same stream (the models of tests/edit_model.py: one oracle decoder per
history), with the taps of fmd_design_lp_kaiser.  Where the channel count is beyond the oracle's reach the expected
rows are those of a small batch of the same process that is itself held against the specification in the same test;
never the output under test.  Geometry: 2.4 MS/s, D 11, 48 kHz (min_samples() == 88, about one audio frame per 50
samples)."""
import ctypes as C

import numpy as np
import pytest

import edit_model as em
import feed_spec as fs
from __graft_entry__ import load_package
from test_gpu_reset_channels import SHIFTS0, _params

pytestmark = pytest.mark.gpu

N = 65536
FILL16 = 0x5A5A
FILL32 = 0x5A5A5A5A
KEEP = "keep"
FMD_ERR_ARG, FMD_ERR_STATE = -1, -4
SHIFTS130 = [int(x) for x in np.resize(np.array(SHIFTS0[:4], np.int32), 130)]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def feed_taps(pkg, Dv, rate=48000.0):
    """the contract's taps, from the design function (not from the batch under test)"""
    f = np.float32(rate)
    fo = np.float32(f / np.float32(Dv))
    return pkg.design_lp_kaiser(1.0, 60.0, float(np.float32(0.425) * fo), float(np.float32(0.575) * fo), float(f))


def walk(state, n, fs_if=em.FS, D=em.D, rate=48000.0):
    """(audio frames of a call of n samples, the state behind it): the decimator phase and the resampler walk of the
    reference (DownConvert.cpp:112-132, 203-232) in float32, as the batch's host plan replays them"""
    step = np.float32(float(np.float32(fs_if / D)) / rate)
    pos, p = state
    M = (n - pos + D - 1) // D
    A, pf = 0, p
    while int(pf) < M:
        A += 1
        pf = np.float32(p + np.float32(np.float32(A) * step))
    return A, (pos + M * D - n, max(np.float32(pf - np.float32(M)), np.float32(0.0)))


def frames_of(sizes):
    """audio frames of every call of a fresh decoder"""
    state, out = (0, np.float32(0.0)), []
    for n in sizes:
        A, state = walk(state, n)
        out.append(A)
    return out


def ragged_sizes(Dv, T):
    """Twelve call sizes for divisor Dv that put into one stream: a call of min_samples() (0 or 1 feed samples); a call
    of fewer frames than the filter has history rows (the roll's overlapping form); calls that start at every g mod
    Dv; calls that deliver 7, 8, 9, 63, 64 and 65 feed samples (the 16-byte groups of both formats and the tile edge);
    and a full call (several tiles).  Found by walking the host plan."""
    sizes, state, g = [], (0, np.float32(0.0)), 0

    def extend(pred, start):
        nonlocal state, g
        for n in range(start, start + 4000):
            A, behind = walk(state, n)
            if pred(g, A):
                sizes.append(n)
                state, g = behind, g + A
                return
        raise AssertionError("no call size found")

    extend(lambda g0, A: True, 88)
    extend(lambda g0, A: True, 1500)

    for r in range(Dv):  # the next call starts at g = r mod Dv
        extend(lambda g0, A, r=r: (g0 + A) % Dv == r and A >= 3, 150 + 50 * r)
    for want in (7, 8, 9, 63, 64, 65):
        extend(lambda g0, A, want=want: fs.count(g0, A, Dv) == want, max(88, (want * Dv - Dv) * 50 - 100))
    while len(sizes) < 11:
        extend(lambda g0, A: True, 333)
    extend(lambda g0, A: True, N)
    assert len(sizes) == 12 and sizes[0] == 88 and sizes[-1] == N
    return sizes


class _Rows:
    """pre-filled output rows on the device: [R, stride] elements, int16 or 32-bit (float rows read as their bits)"""

    def __init__(self, R, stride, s16):
        import torch
        self.s16 = bool(s16)
        self.t = torch.full((max(R, 1), stride), FILL16 if self.s16 else FILL32,
                            dtype=torch.int16 if self.s16 else torch.int32, device="cuda")
        torch.cuda.current_stream().synchronize()

    def ptr(self):
        return self.t.data_ptr()

    def host(self, n_rows, m):
        """(rows [0, n_rows) x [0, m) in the format, whether everything else still holds the fill)"""
        a = self.t.cpu().numpy()
        fill = FILL16 if self.s16 else FILL32
        clean = bool((a[:n_rows, m:] == fill).all()) and bool((a[n_rows:] == fill).all())
        got = a[:n_rows, :m].copy()
        return (got if self.s16 else got.view(np.float32)), clean


def _status_tuple(b, c):
    s = b.status(c)
    vals = (s.tuning_offset, s.interface_level, s.baseband_level, s.pilot_level) + tuple(b.audio_level(c))
    return (s.stereo_detected, s.rds_state) + tuple(int(np.float32(v).view(np.uint32)) for v in vals)


def _apply(b, edit, st):
    import torch
    kind, a = edit[0], edit[1:]
    if kind == "reset":
        b.reset_channels(list(a[0]))
    elif kind == "retune":
        b.retune(list(a[0]), list(a[1]), captures=list(a[2]) if len(a) > 2 else None)
    elif kind == "switch":
        b.switch_captures(list(a[0]), list(a[1]))
    elif kind == "save_load":  # the saved state loaded back into the running batch
        b.wait(stream=st)
        torch.cuda.synchronize()
        b.load_state(b.save_state())
    elif kind == "set_feed":
        b.set_feed(a[0])
    else:
        raise ValueError(kind)


def play(pkg, shifts, streams, script, Dv, plan, cmaps=None, mode=1, lag=0, debug=None, enable=False, skip_roll=False,
         status=False, state=False, pad_rows=1, big=False):
    """One batch with device buffers through `script` ((samples, [edits in front of the call]) as tests/edit_model.py
    writes them, plus ("set_feed", divisor)).  plan[k]: None -- the call has no feed (d_feed == NULL) -- or {"fmt":
    np.int16 / np.float32, "sel": a list, None = one row per channel, KEEP} of call k.  Every call's feed goes to
    pre-filled rows of its own (pad_rows rows and 24 elements more than needed) that are read once
    fmd_batch_wait_lagged(lag) covers the call.  Returns per call the float audio, the delivered feed rows, the
    count, the selection and whether everything else in the rows still holds the fill; optionally the status tuples
    of every call, the groups, and the saved state behind the last call."""
    import torch
    Cn = len(shifts)
    b = pkg.Batch(_params(pkg), Cn, tuning_shifts=np.array(shifts, np.int32), record_callbacks=False)
    if enable:
        b.enable_retune()
    for key, v in (debug or {}).items():
        b.debug_set(key, v)
    b.set_concurrency(mode)
    if cmaps is not None:
        b.set_capture_map(cmaps, streams.G)
    if Dv:
        b.set_feed(Dv)
        assert b.feed() == Dv and b.feed_rate() == 48000.0 / Dv
        assert np.array_equal(b.feed_taps().view(np.uint32), feed_taps(pkg, Dv).view(np.uint32))
    if skip_roll:
        b.debug_feed_skip_roll(1)
    st = torch.cuda.current_stream().cuda_stream
    a_stride = (b.max_audio_floats(N) + 7) // 8 * 8
    f_stride = (max(b.max_feed_samples(N), 1) + 7) // 8 * 8 + 24
    res, keep, pend = [None] * len(script), [], []
    consumed, pos = 0, 0

    def consume(upto):
        nonlocal consumed
        for k in range(consumed, upto):
            out, nf, rows, nfeed, sel = pend[k]
            r = {"audio": None if big else out[:, :nf].cpu().numpy(), "feed": None, "nfeed": nfeed, "sel": sel,
                 "clean": True}
            if rows is not None:
                r["feed"], r["clean"] = rows.host(len(sel), nfeed)
            res[k] = r
            pend[k] = None
        consumed = max(consumed, upto)

    for k, (n, edits) in enumerate(script):
        for e in edits:
            _apply(b, e, st)
        step = plan[k]
        if step is not None and step.get("sel", KEEP) is not KEEP:
            b.select_feed(step["sel"])
        x = streams.block(pos, n)
        pos += n
        if n % 2:  # rows start on a pair of IQ samples
            x = np.concatenate([x, np.zeros((x.shape[0], 2), x.dtype)], axis=1)
        d_iq = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        keep.append(d_iq)
        iq_stride = x.shape[1] // 2 if (streams.G > 1 or cmaps is not None) else 0
        out = torch.zeros((Cn, a_stride), dtype=torch.float32, device="cuda")
        if step is None:
            nf = b.process_device(d_iq.data_ptr(), iq_stride, n, out.data_ptr(), a_stride, st, fmt=pkg.FMD_IQ_F32)
            pend.append((out, nf, None, 0, []))
        else:
            sel = b.feed_selection()
            rows = _Rows(len(sel) + pad_rows, f_stride, np.dtype(step["fmt"]) == np.int16)
            nf, nfeed = b.process_device(d_iq.data_ptr(), iq_stride, n, out.data_ptr(), a_stride, st,
                                         fmt=pkg.FMD_IQ_F32, d_feed_ptr=rows.ptr(), feed_stride=f_stride,
                                         feed=step["fmt"])
            assert nfeed <= b.max_feed_samples(n)
            pend.append((out, nf, rows, nfeed, sel))
        if mode == 2 and not status:
            if k >= lag:
                b.wait(stream=st, lag=lag)
                torch.cuda.current_stream().synchronize()
                consume(k - lag + 1)
        else:
            b.wait(stream=st)
            torch.cuda.synchronize()
            consume(k + 1)
            if status:
                res[k]["status"] = [_status_tuple(b, c) for c in range(Cn)]
    b.wait(stream=st)
    torch.cuda.synchronize()
    consume(len(script))
    extra = {"groups": np.sort(b.collect_rds_array(cap=1 << 18, stream=st, run_group_decoder=False),
                               order=["channel", "call_index"])}
    if state:
        extra["state"] = bytes(b.save_state())
    b.close()
    return res, extra


_MODELS = {}


def model_audio(oracle, streams, script, shifts, cmaps, key):
    """want(k) -> [C, 2 A] float32: every slot's audio in call k from the oracle model of tests/edit_model.py (the
    script without what the model does not know: the feed's own setup call)"""
    if key not in _MODELS:
        clean = [(n, [e for e in edits if e[0] != "set_feed"]) for n, edits in script]
        _MODELS[key] = em.Model(oracle, streams, clean, shifts, cmaps, taps=())
    m = _MODELS[key]

    def want(k, channels=None):
        ch = range(m.C[0]) if channels is None else channels
        return np.stack([m.at(k, c)["audio"] for c in ch])
    return want


def same(got, want_float, what):
    """delivered feed rows against the specification's floats: the bits (float rows) or s16() of them"""
    want_float = np.ascontiguousarray(want_float, np.float32)
    got = np.ascontiguousarray(got)
    assert got.shape == want_float.shape, (what, got.shape, want_float.shape)
    if got.dtype == np.int16:
        g, w = got.astype(np.int64), fs.s16(want_float).astype(np.int64)
    else:
        g, w = got.view(np.uint32).astype(np.int64), want_float.view(np.uint32).astype(np.int64)
    bad = np.argwhere(g != w)
    assert bad.size == 0, (what, len(bad), [(int(r), int(i), int(g[r, i]), int(w[r, i])) for r, i in bad[:6]])


def check_feed(res, plan, want_audio, taps, Dv, Cn, what, restart_at=()):
    """every feed call's rows against the specification over the audio of the feed calls alone (`restart_at`: calls
    with a fmd_batch_set_feed in front of them, where history and g start again)"""
    spec = fs.FeedSpec(taps, Dv, rows=Cn)
    counts = []
    for k, r in enumerate(res):
        if k in restart_at:
            spec = fs.FeedSpec(taps, Dv, rows=Cn)
        if plan[k] is None:
            assert r["feed"] is None and r["nfeed"] == 0
            continue
        y = spec.push(want_audio(k)[:Cn])
        assert r["clean"], (what, k, "something was written outside the rows' samples")
        if len(r["sel"]) == 0:
            assert r["nfeed"] == 0, (what, k)
            continue
        counts.append(r["nfeed"])
        assert r["nfeed"] == y.shape[1], (what, k, r["nfeed"], y.shape[1])
        same(r["feed"], y[r["sel"]], (what, k))
    return counts


def same_audio(res, want_audio, Cn, what):
    for k, r in enumerate(res):
        w = want_audio(k)[:Cn]
        assert r["audio"].shape == w.shape and np.array_equal(r["audio"].view(np.uint32), w.view(np.uint32)), (what, k)


# ---------------------------------------------------------------------------------------------------------------
# 1. wave edges and ragged calls

@pytest.fixture(scope="module")
def ragged(pkg, oracle, fmsig):
    """per divisor: the twelve sizes, the stream and the model's audio of the 130 channels (four tuner shifts)"""
    out = {}
    for Dv in (2, 3):
        sizes = ragged_sizes(Dv, feed_taps(pkg, Dv).size)
        script = [(n, []) for n in sizes]
        streams = em.main_streams(fmsig, em.total_samples(script))
        out[Dv] = (script, streams, model_audio(oracle, streams, script, SHIFTS130, None, ("ragged", Dv)))
    return out


def _ragged_run(pkg, ragged, Cn, Dv, fmt, **kw):
    script, streams, want = ragged[Dv]
    plan = [{"fmt": fmt}] * len(script)
    res, _ = play(pkg, SHIFTS130[:Cn], streams, script, Dv, plan, **kw)
    return script, plan, want, res


@pytest.mark.parametrize("fmt", [np.int16, np.float32], ids=["s16", "f32"])
@pytest.mark.parametrize("Dv", [2, 3])
@pytest.mark.parametrize("Cn", [1, 63, 65, 130])
def test_ragged_calls_equal_the_specification(pkg, ragged, Cn, Dv, fmt):
    script, plan, want, res = _ragged_run(pkg, ragged, Cn, Dv, fmt)
    taps = feed_taps(pkg, Dv)
    same_audio(res, want, Cn, "the audio beside the feed")
    counts = check_feed(res, plan, want, taps, Dv, Cn, (Cn, Dv))
    # the stream holds what it was built for
    A = [r["audio"].shape[1] // 2 for r in res]
    assert A == frames_of([n for n, _ in script])
    g0 = np.concatenate([[0], np.cumsum(A)])[:-1]
    print("frames", A, "feed samples", counts)
    assert script[0][0] == 88 and A[0] in (1, 2) and counts[0] in (0, 1)
    assert A[1] < taps.size - 1
    assert {int(g) % Dv for g in g0} == set(range(Dv))
    assert {7, 8, 9, 63, 64, 65} <= set(counts) and max(counts) > 2 * 64


def test_refusals_that_need_a_batch(pkg, fmsig):
    """a feed pointer while the feed is off: FMD_ERR_STATE; rows shorter than the call's samples: FMD_ERR_ARG; both
    leave the batch as it was -- the next call delivers what the first call of a fresh feed delivers"""
    import torch
    lib = pkg.lib()
    streams = em.main_streams(fmsig, 2 * N)
    b = pkg.Batch(_params(pkg), 2, tuning_shifts=np.array(SHIFTS0[:2], np.int32), record_callbacks=False)
    st = torch.cuda.current_stream().cuda_stream
    d_iq = torch.from_numpy(streams.block(0, 8192)).cuda()
    out = torch.zeros((2, 1024), dtype=torch.float32, device="cuda")
    rows = _Rows(2, 64, True)
    nf, nm, nfeed = C.c_uint(), C.c_uint(), C.c_uint(5)

    def call(stride):
        return lib.fmd_batch_process_device_feed(b._h, d_iq.data_ptr(), 0, 0, 8192, out.data_ptr(), 0, 1024,
                                                 C.byref(nf), None, 0, 0, C.byref(nm), rows.ptr(), 1, stride,
                                                 C.byref(nfeed), st)
    assert b.feed() == 0 and b.max_feed_samples(8192) == 0 and b.feed_rate() == 0.0 and b.feed_taps().size == 0
    assert call(64) == FMD_ERR_STATE and b"feed is off" in lib.fmd_last_error()
    b.set_feed(3)
    A = frames_of([8192])[0]
    n = fs.count(0, A, 3)
    assert 48 < n <= b.max_feed_samples(8192) <= 64
    assert call(48) == FMD_ERR_ARG and b"feed_channel_stride smaller" in lib.fmd_last_error()
    assert nfeed.value == 0
    assert call(64) == 0 and nfeed.value == n and nf.value == 2 * A
    b.wait(stream=st)
    torch.cuda.synchronize()
    got, clean = rows.host(2, n)
    assert clean
    y = fs.FeedSpec(feed_taps(pkg, 3), 3, rows=2).push(out[:, :2 * A].cpu().numpy())
    same(got, y, "the first call behind two refused ones")
    with pytest.raises(pkg.FmdError):
        b.set_feed(4)
    assert b.feed() == 3
    b.set_feed(0)
    assert b.feed() == 0 and call(64) == FMD_ERR_STATE
    b.close()


# ---------------------------------------------------------------------------------------------------------------
# 2. a call without the feed is a splice

def test_a_call_without_the_feed_is_a_splice(pkg, oracle, fmsig):
    """Calls with d_feed == NULL between feed calls: the feed is the specification over the frames of the feed calls
    alone, and audio, status, audio meter, groups and the saved channel state of every call keep the bits of the run
    of a batch whose feed was never turned on."""
    sizes = [N, 8192, 3663, N, 300, 8192, N, 88, N, N] + [N] * 14
    script = [(n, []) for n in sizes]
    streams = em.main_streams(fmsig, em.total_samples(script))
    shifts = SHIFTS0
    want = model_audio(oracle, streams, script, shifts, None, "splice")
    f = [{"fmt": np.int16}, {"fmt": np.float32}]
    plan = [f[0], None, f[1], f[0], None, None, f[1], f[0], None, f[0]] + [f[0], None, f[1], None, f[1], f[0], None] * 2
    res, extra = play(pkg, shifts, streams, script, 3, plan, status=True, state=True)
    ref, ref_extra = play(pkg, shifts, streams, script, 0, [None] * len(script), status=True, state=True)
    check_feed(res, plan, want, feed_taps(pkg, 3), 3, len(shifts), "splice")
    same_audio(ref, want, len(shifts), "the run without the feed")
    for k in range(len(script)):
        assert np.array_equal(res[k]["audio"].view(np.uint32), ref[k]["audio"].view(np.uint32)), k
        assert res[k]["status"] == ref[k]["status"], k
    assert len(extra["groups"]) > 0 and np.array_equal(extra["groups"], ref_extra["groups"])
    assert extra["state"] == ref_extra["state"]


# ---------------------------------------------------------------------------------------------------------------
# 3. selections

FLIGHT_SIZES = [8192, 4096, N, 3663, 8192, 300, 4096, 8192, 20001, 4096] * 2


def _shapes(Cn):
    rng = np.random.default_rng(Cn)
    return {"empty": [], "one": [Cn // 2], "every-second-reversed": list(range(0, Cn, 2))[::-1],
            "all-shuffled": [int(c) for c in rng.permutation(Cn)], "none": None,
            "strided": list(range(1, Cn, 3))}


def _flight_plan(Cn):
    """20 calls, the selection changed in front of every one; channel 7 is selected for the first time at call 10"""
    shapes, names = _shapes(Cn), list(_shapes(Cn))
    plan = []
    for k in range(20):
        sel = shapes[names[k % len(names)]]
        if k < 10:
            sel = [c for c in (sel if sel is not None else list(range(0, Cn, 5))) if c != 7]
        elif k == 10:
            sel = [7, 64, 3]
        plan.append({"fmt": (np.int16, np.float32)[(k // 3) % 2], "sel": sel})
    return plan


@pytest.fixture(scope="module")
def unselected(pkg, oracle, fmsig):
    """the 20 calls of FLIGHT_SIZES on 130 channels without a selection, one call at a time: held against the
    specification here, and what the selected runs are compared with"""
    script = [(n, []) for n in FLIGHT_SIZES]
    streams = em.main_streams(fmsig, em.total_samples(script))
    want = model_audio(oracle, streams, script, SHIFTS130, None, "flight")
    plan = [{"fmt": np.float32}] * len(script)
    res, _ = play(pkg, SHIFTS130, streams, script, 2, plan)
    check_feed(res, plan, want, feed_taps(pkg, 2), 2, 130, "unselected")
    return script, streams, res


@pytest.mark.parametrize("mode,lag,layout", [(2, 1, 0), (2, 2, 0), (2, 3, 0), (2, 1, 1), (2, 2, 1), (2, 3, 1),
                                             (2, 1, 2), (2, 2, 2), (2, 3, 2), (1, 0, 0), (1, 0, 1), (1, 0, 2),
                                             (0, 0, -1)])
def test_selection_changes_with_calls_in_flight(pkg, unselected, mode, lag, layout):
    """Every selection shape (empty, one, reversed, strided, shuffled, none) changed in front of every one of 20 calls
    in flight, read `lag` calls late, on every stream layout of an overlapped call and in every concurrency mode: row i
    is channel sel[i]'s row of the unselected run, bit for bit (int16 rows: s16() of it); rows >= n and everything
    behind the samples keep their fill; an empty selection delivers nothing and the feed goes on behind it; channel 7,
    selected for the first time at call 10, has its true history."""
    script, streams, ref = unselected
    plan = _flight_plan(130)
    res, _ = play(pkg, SHIFTS130, streams, script, 2, plan, mode=mode, lag=lag,
                  debug={"lpf_late": layout} if layout >= 0 else None)
    seen = set()
    for k, r in enumerate(res):
        want_sel = plan[k]["sel"] if plan[k]["sel"] is not None else list(range(130))
        assert r["sel"].tolist() == want_sel, k
        assert r["clean"], k
        seen.add(len(want_sel))
        if not want_sel:
            assert r["nfeed"] == 0, k
            continue
        assert r["nfeed"] == ref[k]["nfeed"], k
        same(r["feed"], ref[k]["feed"][want_sel], ("selected", k))
    assert 7 in res[10]["sel"] and not any(7 in r["sel"] for r in res[:10])
    assert seen >= {0, 1, 3, 65, 130}


# ---------------------------------------------------------------------------------------------------------------
# 4. edits

def test_edits_leave_the_feed_to_the_output(pkg, oracle, fmsig):
    """Eight channels over two captures, retuning enabled: a reset, a retune (one to a capture) and a capture switch
    of single channels between ragged calls, and a saved state loaded back.  The feed's history and g are the output's:
    it goes on as the specification over the audio the slots now produce (the models of tests/edit_model.py), the
    untouched channels keep their bits.  fmd_batch_set_feed again -- the same divisor -- zeroes history and g."""
    S = em._steps
    script = S(N, N, (88, [("reset", [0, 5])]), 97, (3663, [("retune", [3], [em.OTHER])]), 300,
               (8192, [("switch", [4], [1])]), (150, [("retune", [1], [em.BSIDE], [1])]), N, (1001, [("save_load",)]),
               8192, (8192, [("set_feed", 3)]), (333, [("reset", [2])]), N)
    streams = em.main_streams(fmsig, em.total_samples(script), two=True)
    shifts, cmaps = list(em.SHIFTS_2CAP), [0] * 8
    want = model_audio(oracle, streams, script, shifts, cmaps, "edits")
    plan = [{"fmt": (np.float32, np.int16)[k % 2]} for k in range(len(script))]
    res, _ = play(pkg, shifts, streams, script, 3, plan, cmaps=cmaps, enable=True)
    same_audio(res, want, 8, "the edited decoders' audio")
    check_feed(res, plan, want, feed_taps(pkg, 3), 3, 8, "edits", restart_at=(11,))


# ---------------------------------------------------------------------------------------------------------------
# 5. saturation

def test_over_deviated_station_saturates_like_the_specification(pkg, oracle, fmsig):
    """The over-deviated station of tests/test_gpu_pcm_formats.py (150 kHz of deviation) through a single decoder:
    the int16 rows equal s16() of the specification over the oracle's audio, and the specification itself saturates
    there."""
    fsr, D = 2.4e6, 11
    p = fmsig.default_params(fsr, noise_sigma=0.005, dev=150e3)
    o = oracle.OracleDecoder(fsr, -0.15 * fsr, 48000.0, 15000.0, D)
    d = pkg.FmDecoder(fsr, -0.15 * fsr, 48000.0, 15000.0, D)
    d.SetFeed(2)
    spec = fs.FeedSpec(feed_taps(pkg, 2), 2)
    ys = []
    for blk in range(6):
        x = fmsig.generate_f32(p, blk * N, N)
        ref = o.process_stream(x)
        audio, feed = d.ProcessStreamWithFeed(x.view(np.complex64), feed=np.int16)
        assert np.array_equal(audio.view(np.uint32), ref.view(np.uint32))
        y = spec.push(ref[None, :])
        same(feed[None, :], y, ("over-deviated", blk))
        ys.append(y[0])
    y = np.concatenate(ys)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(y * np.float32(32768))
    n_sat = int(((r > 32767) | (r < -32768)).sum())
    print("feed samples %d, saturated in the specification %d, peak %.3f" % (y.size, n_sat, float(np.abs(y).max())))
    assert n_sat >= 1


# ---------------------------------------------------------------------------------------------------------------
# 6. sub-batches

def test_feed_across_sub_batches(pkg, oracle, fmsig):
    """A shell of 16 384 channels (two sub-batches, a scratch and a frame count each) on one shared capture, short
    calls: channel c delivers the rows of channel c % 8 of an 8-channel batch that is held against the specification
    here; then a selection that interleaves both sub-batches, and a call without the feed between them."""
    Cn = 16384
    sizes = [8192, 300, 8192, 3663, 8192, 8192]
    script = [(n, []) for n in sizes]
    streams = em.main_streams(fmsig, em.total_samples(script))
    want = model_audio(oracle, streams, script, SHIFTS0, None, "shell")
    inter = [8192 + 5, 3, 16383, 0, 8192, 8191, 12000, 4097]
    plan = [{"fmt": np.int16}, {"fmt": np.float32}, None, {"fmt": np.float32, "sel": inter},
            {"fmt": np.int16, "sel": KEEP}, {"fmt": np.int16, "sel": None}]
    small_plan = [None if s is None else {"fmt": np.float32} for s in plan]
    small, _ = play(pkg, SHIFTS0, streams, script, 3, small_plan)
    check_feed(small, small_plan, want, feed_taps(pkg, 3), 3, 8, "small")
    shifts = [int(x) for x in np.resize(np.array(SHIFTS0, np.int32), Cn)]
    res, _ = play(pkg, shifts, streams, script, 3, plan, big=True)
    for k, r in enumerate(res):
        if plan[k] is None:
            continue
        assert r["clean"], k
        sel = r["sel"]
        assert sel.tolist() == (inter if k in (3, 4) else list(range(Cn))), k
        assert r["nfeed"] == small[k]["nfeed"], k
        same(r["feed"], small[k]["feed"][sel % 8], ("shell", k))


# ---------------------------------------------------------------------------------------------------------------
# 7. single decoder and host entry points

def test_host_entry_points_take_any_stride(pkg, oracle, fmsig):
    """fmd_batch_process_host_feed into rows of an odd stride that start on an odd element, both formats, with and
    without a selection; Batch.process_host_fmt(feed=...) beside the multiplex; FmDecoder.ProcessStreamWithFeed."""
    lib = pkg.lib()
    sizes = [N, 8191, 300, N]
    script = [(n, []) for n in sizes]
    streams = em.main_streams(fmsig, em.total_samples(script))
    shifts = SHIFTS0[:5]
    want = model_audio(oracle, streams, script, shifts, None, "host")
    taps = feed_taps(pkg, 3)
    spec = fs.FeedSpec(taps, 3, rows=5)
    b = pkg.Batch(_params(pkg), 5, tuning_shifts=np.array(shifts, np.int32), record_callbacks=False)
    b.set_feed(3)
    stride = (b.max_feed_samples(N) + 3) | 1
    pos = 0
    for k, n in enumerate(sizes):
        x = streams.block(pos, n)[0]
        pos += n
        y = spec.push(want(k))
        s16 = k % 2 == 0
        sel = [4, 0, 2] if k >= 2 else list(range(5))
        if k == 2:
            b.select_feed(sel)
        if k == 1:  # the wrapper, the multiplex beside the feed
            audio, mpx, feed = b.process_host_fmt(x, shared=True, mpx=np.float32, feed=np.float32)
            assert mpx.shape[0] == 5 and mpx.shape[1] > 0
            same(feed, y, ("wrapper", k))
            assert np.array_equal(audio.view(np.uint32), want(k).view(np.uint32))
            continue
        raw = np.full(len(sel) * stride + 9, FILL16 if s16 else FILL32, np.int16 if s16 else np.int32)
        rows = raw[1:]  # (an odd element: 2 or 4 bytes off any 16-byte boundary)
        audio = np.zeros((5, b.max_audio_floats(n)), np.float32)
        nf, nm, nfeed = C.c_uint(), C.c_uint(), C.c_uint()
        rc = lib.fmd_batch_process_host_feed(b._h, x.ctypes.data, 0, 0, n, audio.ctypes.data, 0, audio.shape[1],
                                             C.byref(nf), None, 0, 0, C.byref(nm), rows.ctypes.data, int(s16), stride,
                                             C.byref(nfeed))
        assert rc >= 0, lib.fmd_last_error()
        assert nfeed.value == y.shape[1] and nm.value == 0
        got = rows[:len(sel) * stride].reshape(len(sel), stride)
        assert (got[:, nfeed.value:] == (FILL16 if s16 else FILL32)).all() and raw[0] == (FILL16 if s16 else FILL32)
        assert (rows[len(sel) * stride:] == (FILL16 if s16 else FILL32)).all()
        got = got[:, :nfeed.value].copy()
        same(got if s16 else got.view(np.float32), y[sel], ("host", k))
        assert np.array_equal(audio[:, :nf.value].view(np.uint32), want(k).view(np.uint32))
    b.close()
    # the single decoder: a tuner of its own (no shift table), so its audio is compared with a second decoder's
    d, plain = (pkg.FmDecoder(em.FS, -0.15 * em.FS, 48000.0, 15000.0, em.D) for _ in range(2))
    with pytest.raises(pkg.FmdError):
        d.ProcessStreamWithFeed(streams.block(0, 8192)[0].view(np.complex64))  # the feed is off
    d.SetFeed(2)
    spec = fs.FeedSpec(feed_taps(pkg, 2), 2)
    pos = 0
    for k, n in enumerate([N, 8192, N]):
        x = streams.block(pos, n)[0].view(np.complex64)
        pos += n
        audio, feed = d.ProcessStreamWithFeed(x, feed=(np.int16, np.float32)[k % 2])
        ref = plain.ProcessStream(x)
        assert np.array_equal(audio.view(np.uint32), ref.view(np.uint32))
        same(feed[None, :], spec.push(ref[None, :]), ("decoder", k))


# ---------------------------------------------------------------------------------------------------------------
# 8. teeth

def test_a_stale_history_fails_at_the_first_call_boundary(pkg, ragged):
    """With fmd_batch_debug_feed_skip_roll the history rows stay what fmd_batch_set_feed left (zeros).  The ragged
    stream's check then fails, and it fails exactly where it has to: the rows equal the specification with every
    call's history zeroed, whose first difference from the real one is the first sample whose taps reach back over a
    call boundary onto a frame that is not zero -- nothing before it differs."""
    Dv, Cn = 3, 65
    script, plan, want, res = _ragged_run(pkg, ragged, Cn, Dv, np.float32, skip_roll=True)
    taps = feed_taps(pkg, Dv)
    with pytest.raises(AssertionError):
        check_feed(res, plan, want, taps, Dv, Cn, "stale history")
    spec, g0, first_dev, first_stale = fs.FeedSpec(taps, Dv, rows=Cn), 0, None, None
    for k, r in enumerate(res):
        audio = want(k)[:Cn]
        y = spec.push(audio)
        x = fs.mono(audio)
        A = x.shape[1]
        first = -((-g0) // Dv)
        stale = fs.outputs(np.concatenate([np.zeros((Cn, g0), np.float32), x], axis=1), taps, Dv, first,
                           fs.count(g0, A, Dv))
        assert r["nfeed"] == y.shape[1] == stale.shape[1]
        same(r["feed"], stale, ("the specification over a zeroed history", k))
        for got, which in ((r["feed"], "dev"), (stale, "stale")):
            bad = np.argwhere(got.view(np.uint32) != y.view(np.uint32))
            if bad.size and which == "dev" and first_dev is None:
                first_dev = (k, int(bad[:, 1].min()), g0)
            if bad.size and which == "stale" and first_stale is None:
                first_stale = (k, int(bad[:, 1].min()), g0)
        g0 += A
    assert first_dev is not None and first_dev == first_stale
    k, j, g0 = first_dev
    n = -((-g0) // Dv) + j  # the sample's index in the feed
    print("first wrong sample: call %d, sample %d of it (feed sample %d at frame %d; the call starts at frame %d)"
          % (k, j, n, n * Dv, g0))
    assert k >= 1 and n * Dv - (taps.size - 1) < g0, "the sample does not reach back over its call's first frame"
