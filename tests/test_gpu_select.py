"""Which channels a batch delivers audio and multiplex rows for (fmd_batch_select_audio / _mpx, include/fmd.h, DESIGN.md
section 9.9): row i of the output is channel channels[i], the call writes exactly n rows, and nothing else moves.

No tolerance: a selected row is bit for bit the row the unselected call writes.  Expected values are the CPU oracle's
audio and `baseband` tap (pcm16() / mpx16() of them for the 16-bit formats); where the channel count is beyond the
oracle's reach they are the rows of an unselected batch of the same process fed the same input -- the path a batch
without a selection always took, itself compared with the oracle in the same test at 130 channels.  Never the selected
output itself.  Every comparison is an equality."""
import ctypes as C

import numpy as np
import pytest

from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

N = 65536
FILL16 = 0x5A5A
FILL32 = 0x5A5A5A5A
FS, D = 2.4e6, 11
KEEP = "keep"  # a plan entry that leaves the selection as it is


def pcm16(x):
    y = np.asarray(x, np.float32) * np.float32(32768.0)
    with np.errstate(invalid="ignore"):
        r = np.clip(np.rint(y), -32768.0, 32767.0)
    return np.where(np.isnan(y), 0, r).astype(np.int16)


def mpx16(x):
    y = np.asarray(x, np.float32) * np.float32(8192.0)
    with np.errstate(invalid="ignore"):
        r = np.clip(np.rint(y), -32768.0, 32767.0)
    return np.where(np.isnan(y), 0, r).astype(np.int16)


def clipped(x):
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(np.asarray(x, np.float32) * np.float32(32768))
        return (r > 32767) | (r < -32768)


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def _same(got, want_float, conv, what):
    """delivered rows against expected floats: the bits (float rows) or conv() of them (int16 rows)"""
    want_float = np.ascontiguousarray(want_float, np.float32)
    got = np.ascontiguousarray(got)
    if got.dtype == np.int16:
        g, w = got.reshape(-1).astype(np.int64), conv(want_float).reshape(-1).astype(np.int64)
    else:
        g, w = got.view(np.uint32).reshape(-1).astype(np.int64), want_float.view(np.uint32).reshape(-1).astype(np.int64)
    assert got.shape == want_float.shape, (what, got.shape, want_float.shape)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (what, bad.size, [(int(i), int(g[i]), int(w[i])) for i in bad[:6]])


def _station(fmsig, **kw):
    return fmsig.default_params(FS, noise_sigma=0.005, **kw)


def _shifts(Cn):
    return np.array([(10, 9, 10, 11)[c % 4] for c in range(Cn)], np.int32)


def _status_tuple(b, c):
    s = b.status(c)
    vals = (s.tuning_offset, s.interface_level, s.baseband_level, s.pilot_level) + tuple(b.audio_level(c))
    return (s.stereo_detected, s.rds_state) + tuple(int(np.float32(v).view(np.uint32)) for v in vals)


_BLOCKS = {}


def _shared_rows(fmsig, sizes, **kw):
    """the blocks of one station, call after call: [1, 2 n] float IQ each (computed once per stream)"""
    key = (tuple(sizes), tuple(sorted(kw.items())))
    if key not in _BLOCKS:
        p, rows, start = _station(fmsig, **kw), [], 0
        for n in sizes:
            rows.append(fmsig.generate_f32(p, start, n)[None, :])
            start += n
        _BLOCKS[key] = rows
    return _BLOCKS[key]


_ORACLE = {}


def _oracle_rows(oracle, shift, rows, key):
    """(audio, baseband tap) of every call of the oracle decoder with tuner shift `shift` on capture row 0 of `rows`
    (once per stream and shift)"""
    key = (key, int(shift))
    if key not in _ORACLE:
        o = oracle.OracleDecoder(FS, 0.0, 48000.0, 15000.0, D, tuning_shift=int(shift))
        out = []
        for r in rows:
            a = o.process_stream(r[0]).copy()
            out.append((a, o.taps()["baseband"].copy()))
        _ORACLE[key] = out
    return _ORACLE[key]


class _Rows:
    """pre-filled output rows on the device: [R, stride] elements, int16 or 32-bit (float rows read as their bits)"""

    def __init__(self, R, stride, s16):
        import torch
        self.s16 = bool(s16)
        self.t = torch.empty((max(R, 1), stride), dtype=torch.int16 if self.s16 else torch.int32, device="cuda")
        self.stride = stride
        self.fill()

    def fill(self):
        import torch
        self.t.fill_(FILL16 if self.s16 else FILL32)
        torch.cuda.current_stream().synchronize()  # (this stream only: calls in flight stay in flight)

    def ptr(self):
        return self.t.data_ptr()

    def host(self, n_rows, m):
        """(rows [0, n_rows) x [0, m) in the format, whether everything else still holds the fill)"""
        a = self.t.cpu().numpy()
        fill = FILL16 if self.s16 else FILL32
        clean = bool((a[:n_rows, m:] == fill).all()) and bool((a[n_rows:] == fill).all())
        got = a[:n_rows, :m].copy()
        return (got if self.s16 else got.view(np.float32)), clean


def _is16(fmt):
    return fmt is not None and np.dtype(fmt) == np.int16


def _run(pkg, Cn, shifts, rows, sizes, plan, mode=2, lag=2, nbuf=6, setup=None, edit=None, cmap=None,
         every_status=False, callbacks=False, pad_rows=1):
    """One batch with device buffers, calls submitted back to back.  plan[k]: {"a": audio selection, "m": multiplex
    selection (a list, None = one row per channel, KEEP), "pcm": audio format, "mpx": multiplex format or None} of
    call k; the selections are applied in front of the call.  Call k's outputs go to rotating pre-filled buffers of
    Cn + pad_rows rows and over-long strides and are read as soon as fmd_batch_wait_lagged(lag) covers the call.
    Returns per call the delivered audio and multiplex rows with whether everything else in their buffers still holds
    the fill, the selections as the getters reported them, status tuples, groups, frames and names."""
    import torch
    b = pkg.Batch(pkg.make_params(FS, -0.15 * FS, 48000.0, 15000.0, D), Cn, tuning_shifts=shifts,
                  record_callbacks=callbacks)
    b.set_concurrency(mode)
    if setup:
        setup(b)
    if cmap is not None:
        b.set_capture_map(cmap, rows[0].shape[0])
    st = torch.cuda.current_stream().cuda_stream
    a_stride = (b.max_audio_floats(max(sizes)) + 7) // 8 * 8 + 24
    m_stride = (b.max_mpx_samples(max(sizes)) + 7) // 8 * 8 + 24
    R = Cn + pad_rows
    ring = [{} for _ in range(nbuf)]

    def buf(k, kind, s16):
        key = (kind, s16)
        if key not in ring[k % nbuf]:
            ring[k % nbuf][key] = _Rows(R, a_stride if kind == "a" else m_stride, s16)
        elif k >= nbuf:
            ring[k % nbuf][key].fill()
        return ring[k % nbuf][key]

    keep, used, nfs, nms, sel_a, sel_m = [], [], [], [], [], []
    res = [None] * len(sizes)
    status, consumed = {}, 0
    cur_a, cur_m = None, None

    def consume(upto):  # calls [consumed, upto) are complete
        nonlocal consumed
        for k in range(consumed, upto):
            ab, mb = used[k]
            na, nm_rows = len(sel_a[k]), len(sel_m[k])
            a, a_clean = ab.host(na, nfs[k])
            m, m_clean = (None, True) if mb is None else mb.host(nm_rows, nms[k])
            res[k] = {"a": a, "a_clean": a_clean, "m": m, "m_clean": m_clean}
        consumed = max(consumed, upto)

    for k, n in enumerate(sizes):
        step = plan[k]
        if edit:
            edit(b, k)
        if step.get("a", KEEP) is not KEEP:
            b.select_audio(step["a"])
            cur_a = step["a"]
        if step.get("m", KEEP) is not KEEP:
            b.select_mpx(step["m"])
            cur_m = step["m"]
        sel_a.append(b.audio_selection())
        sel_m.append(b.mpx_selection())
        assert sel_a[-1].tolist() == (list(range(Cn)) if cur_a is None else [int(c) for c in cur_a])
        assert sel_m[-1].tolist() == (list(range(Cn)) if cur_m is None else [int(c) for c in cur_m])
        n_al = (n + 1) // 2 * 2
        x = np.zeros((rows[k].shape[0], 2 * n_al), np.float32)
        x[:, :2 * n] = rows[k]
        d_iq = torch.from_numpy(x).cuda()
        keep.append(d_iq)
        iq_stride = n_al if (cmap is not None or rows[k].shape[0] > 1) else 0
        pcm, mfmt = step.get("pcm", np.float32), step.get("mpx", None)
        assert k < nbuf or consumed > k - nbuf  # the buffers' last call has been read
        ab = buf(k, "a", _is16(pcm))
        mb = buf(k, "m", _is16(mfmt)) if mfmt is not None else None
        if mb is None:
            nfs.append(b.process_device(d_iq.data_ptr(), iq_stride, n, ab.ptr(), a_stride, st, fmt=pkg.FMD_IQ_F32,
                                        pcm=pcm))
            nms.append(0)
        else:
            nf, nm = b.process_device(d_iq.data_ptr(), iq_stride, n, ab.ptr(), a_stride, st, fmt=pkg.FMD_IQ_F32,
                                      pcm=pcm, d_mpx_ptr=mb.ptr(), mpx_stride=m_stride, mpx=mfmt)
            nfs.append(nf)
            nms.append(nm)
        used.append((ab, mb))
        if mode == 2 and not every_status:
            if k >= lag:
                b.wait(stream=st, lag=lag)
                torch.cuda.current_stream().synchronize()
                consume(k - lag + 1)
        else:
            b.wait(stream=st)
            torch.cuda.synchronize()
            consume(k + 1)
            if every_status:
                status[k] = [_status_tuple(b, c) for c in range(Cn)]
    b.wait(stream=st)
    torch.cuda.synchronize()
    consume(len(sizes))
    status["end"] = [_status_tuple(b, c) for c in range(0, Cn, max(1, Cn // 64))]
    groups = b.collect_rds_array(cap=1 << 18, stream=st, run_group_decoder=callbacks)
    out = {"calls": res, "nf": nfs, "nm": nms, "sel_a": sel_a, "sel_m": sel_m, "status": status,
           "groups": np.sort(groups, order=["channel", "call_index"]),
           "frames": dict(b.sink.frames) if callbacks else None, "names": dict(b.sink.names) if callbacks else None,
           "clipped": b.pcm_clipped()}
    b.close()
    return out


def _baseband_lengths(sizes):
    pos, out = 0, []
    for n in sizes:
        m = (n - pos + D - 1) // D
        out.append(m)
        pos = pos + m * D - n
    return out


def _check_against(r, plan, want_a, want_m, what):
    """every call's delivered rows against want_a(k, channels) / want_m(k, channels): float rows [len(channels), .]"""
    for k, c in enumerate(r["calls"]):
        assert c["a_clean"] and c["m_clean"], (what, k, c["a_clean"], c["m_clean"])
        ch = r["sel_a"][k]
        assert c["a"].shape[0] == ch.size, (what, k)
        if ch.size:
            _same(c["a"], want_a(k, ch), pcm16, (what, "audio", k))
        if plan[k].get("mpx") is not None:
            ch = r["sel_m"][k]
            assert c["m"].shape[0] == ch.size, (what, k)
            if ch.size:
                assert r["nm"][k] == want_m(k, ch).shape[1]
                _same(c["m"], want_m(k, ch), mpx16, (what, "multiplex", k))


def _by_shift(oracle, shifts, rows, key, which):
    """want(k, channels): the oracle's rows of the channels' tuner shifts on the shared capture"""
    def want(k, ch):
        return np.stack([_oracle_rows(oracle, shifts[c], rows, key)[k][which] for c in ch])
    return want


def _of_batch(ref, which):
    """want(k, channels): the float rows of an unselected batch's call k"""
    def want(k, ch):
        return ref["calls"][k][which][ch]
    return want


# ---------------------------------------------------------------------------------------------------------------
# 1. batch sizes and selection shapes

def _shapes(Cn):
    rng = np.random.default_rng(Cn)
    return {"empty": [], "one": [Cn // 2], "every-second-reversed": list(range(0, Cn, 2))[::-1],
            "all-shuffled": [int(c) for c in rng.permutation(Cn)], "none": None}


@pytest.mark.parametrize("Cn", [1, 63, 65, 130])
def test_selected_rows_equal_the_oracles(pkg, oracle, fmsig, Cn):
    """Batches that end inside a wave, at a wave and behind it, on a shared capture with four tuner shifts; every
    selection shape for both outputs, both audio and both multiplex formats, the two selections different in every
    call; calls of 8192 and 65 536 samples (baseband lengths that end inside a 16-byte group and inside a tile).
    Every delivered row is the oracle's; behind a row's samples and in rows >= n the buffers hold their fill."""
    sizes = [8192, N, 8192, 8192, N, 8192]
    rows, shifts = _shared_rows(fmsig, sizes), _shifts(Cn)
    names = list(_shapes(Cn))
    plan = []
    for k in range(len(sizes)):
        plan.append({"a": _shapes(Cn)[names[k % 5]], "m": _shapes(Cn)[names[(k + 2) % 5]],
                     "pcm": (np.float32, np.int16)[k % 2], "mpx": (np.float32, np.int16)[(k // 2) % 2]})
    plan[5]["a"], plan[5]["m"] = _shapes(Cn)["every-second-reversed"], _shapes(Cn)["all-shuffled"]
    r = _run(pkg, Cn, shifts, rows, sizes, plan, mode=1)
    want_m = _baseband_lengths(sizes)
    assert [r["nm"][k] for k in range(len(sizes)) if len(r["sel_m"][k])] == \
        [want_m[k] for k in range(len(sizes)) if len(r["sel_m"][k])]
    assert [r["nm"][k] for k in range(len(sizes)) if not len(r["sel_m"][k])] == [0]  # an empty selection: no multiplex
    _check_against(r, plan, _by_shift(oracle, shifts, rows, "shapes", 0), _by_shift(oracle, shifts, rows, "shapes", 1),
                   Cn)
    seen_a = {(len(r["sel_a"][k]), _is16(plan[k]["pcm"])) for k in range(len(sizes))}
    assert {n for n, _ in seen_a} >= {0, 1, Cn, (Cn + 1) // 2}


# ---------------------------------------------------------------------------------------------------------------
# 2. everything else keeps its bits

def test_everything_else_keeps_its_bits(pkg, fmsig):
    """130 channels of three stations with their own RDS, 24 calls, a selection that changes every other call (empty,
    one row, a reversed half, shuffled) against the same batch without any: status tuple and audio meter of EVERY
    channel after EVERY call, RDS groups with their call index, UECP frames and PS names are identical -- also for the
    channels that deliver nothing."""
    Cn, G = 130, 3
    sizes = [N] * 24
    sts = [_station(fmsig, seed=500 + g, pi=0x5100 + g) for g in range(G)]
    rows, start = [], 0
    for n in sizes:
        rows.append(np.stack([fmsig.generate_f32(sts[g], start, n) for g in range(G)]))
        start += n
    cmap = np.arange(Cn) % G
    names = ["empty", "one", "every-second-reversed", "all-shuffled", "none", "one"]
    plan = [{"a": _shapes(Cn)[names[(k // 2) % 6]], "m": _shapes(Cn)[names[(k // 2 + 1) % 6]],
             "pcm": (np.float32, np.int16)[k % 2], "mpx": (np.int16, np.float32, None)[k % 3]}
            for k in range(len(sizes))]
    plain_plan = [dict(p, a=None, m=None) for p in plan]
    kw = dict(mode=1, cmap=cmap, every_status=True, callbacks=True)
    plain = _run(pkg, Cn, None, rows, sizes, plain_plan, **kw)
    r = _run(pkg, Cn, None, rows, sizes, plan, **kw)
    for k in range(len(sizes)):
        assert r["status"][k] == plain["status"][k], k
    assert r["status"]["end"] == plain["status"]["end"]
    assert len(plain["groups"]) > 100 and np.array_equal(r["groups"], plain["groups"])
    assert len(plain["frames"]) > 0 and r["frames"] == plain["frames"]
    assert r["names"] == plain["names"]
    # and the rows that were delivered are the plain batch's (float rows there: the selected ones are held against
    # pcm16 / mpx16 of them)
    fplan = [dict(p, pcm=np.float32, mpx=np.float32) for p in plain_plan]
    fl = _run(pkg, Cn, None, rows, sizes, fplan, mode=1, cmap=cmap)
    _check_against(r, plan, _of_batch(fl, "a"), _of_batch(fl, "m"), "rows")


# ---------------------------------------------------------------------------------------------------------------
# 3. clip counter

def test_clip_counter_counts_delivered_samples_only(pkg, fmsig):
    """Four channels, two of them the over-deviated station, 10 S16 calls: channels 1 and 2 are selected (one of each
    station), their pcm_clipped equals the numpy count over a float batch's audio; channels 0 and 3 deliver nothing
    and count nothing, although the over-deviated one, 3, saturates (its count in the float audio is not 0)."""
    Cn = 4
    sizes = [N] * 10
    ps = [_station(fmsig, seed=80 + c, **({"dev": 150e3} if c % 2 == 1 else {})) for c in range(Cn)]
    rows, start = [], 0
    for n in sizes:
        rows.append(np.stack([fmsig.generate_f32(ps[c], start, n) for c in range(Cn)]))
        start += n
    fplan = [{"a": None, "pcm": np.float32}] * len(sizes)
    fl = _run(pkg, Cn, None, rows, sizes, fplan, mode=1)
    plan = [{"a": [2, 1] if k == 0 else KEEP, "pcm": np.int16} for k in range(len(sizes))]
    r = _run(pkg, Cn, None, rows, sizes, plan, mode=1)
    want = np.zeros(Cn, np.uint64)
    for k in range(len(sizes)):
        want += clipped(fl["calls"][k]["a"]).sum(axis=1).astype(np.uint64)
        _same(r["calls"][k]["a"], fl["calls"][k]["a"][[2, 1]], pcm16, k)
    assert want[1] > 0 and want[3] > 0
    assert r["clipped"].tolist() == [0, int(want[1]), int(want[2]), 0]
    assert not fl["clipped"].any()


# ---------------------------------------------------------------------------------------------------------------
# 4. calls in flight

_FLIGHT_SIZES = [8192, 16384, 12001, 8192, 20001, 8192, 8193, 16384, 8192, 8192, 30001, 8192, 8192, 16384, 9001, 8192,
                 8192, 12288, 8192, 8192]


def _flight_plan(Cn, n_calls):
    """a different random subset and order in front of every call, empty and None among them"""
    rng = np.random.default_rng(4)
    plan = []
    for k in range(n_calls):
        def pick(j):
            if j % 7 == 3:
                return []
            if j % 7 == 5:
                return None
            return [int(c) for c in rng.permutation(Cn)[:int(rng.integers(1, Cn + 1))]]
        plan.append({"a": pick(k), "m": pick(k + 2), "pcm": (np.int16, np.float32)[k % 2],
                     "mpx": (np.float32, np.int16)[(k // 3) % 2]})
    return plan


@pytest.fixture(scope="module")
def serial_flight(pkg, fmsig):
    """the 130-channel batch in serial mode (everything on the caller's stream) given the same sequence"""
    rows = _shared_rows(fmsig, _FLIGHT_SIZES)
    return _run(pkg, 130, _shifts(130), rows, _FLIGHT_SIZES, _flight_plan(130, len(_FLIGHT_SIZES)), mode=0)


@pytest.mark.parametrize("lag", [1, 2, 3])
@pytest.mark.parametrize("how", ["default", "split_post", "lpf_late0", "lpf_late1", "lpf_late2"])
def test_selections_of_calls_in_flight(pkg, oracle, fmsig, serial_flight, how, lag):
    """130 channels, concurrency 2, 20 calls (2 x NSLOT + 4: every table version is reused under readers) into 6
    rotating pre-filled buffers, both selections changed in front of EVERY call, each call read as soon as
    fmd_batch_wait_lagged(lag) covers it: every call delivers the rows of the selection it was submitted with -- the
    concurrency-0 batch's for the same sequence, and both the oracle's --, with the post chain on two streams and with
    each stream layout."""
    Cn, sizes = 130, _FLIGHT_SIZES
    assert len(sizes) >= 2 * 8 + 2
    rows, shifts = _shared_rows(fmsig, sizes), _shifts(Cn)
    plan = _flight_plan(Cn, len(sizes))
    setup = {"default": None, "split_post": lambda b: b.debug_set("split_post", 1),
             "lpf_late0": lambda b: b.debug_set("lpf_late", 0), "lpf_late1": lambda b: b.debug_set("lpf_late", 1),
             "lpf_late2": lambda b: b.debug_set("lpf_late", 2)}[how]
    r = _run(pkg, Cn, shifts, rows, sizes, plan, mode=2, lag=lag, nbuf=6, setup=setup)
    want_a, want_m = _by_shift(oracle, shifts, rows, "flight", 0), _by_shift(oracle, shifts, rows, "flight", 1)
    _check_against(serial_flight, plan, want_a, want_m, "serial against the oracle")
    _check_against(r, plan, want_a, want_m, "in flight against the oracle")
    for k in range(len(sizes)):
        for key in ("a", "m"):
            g, w = r["calls"][k][key], serial_flight["calls"][k][key]
            assert (g is None and w is None) or (g.dtype == w.dtype and np.array_equal(g.view(np.uint16),
                                                                                     w.view(np.uint16))), (k, key)
    assert r["nf"] == serial_flight["nf"] and r["nm"] == serial_flight["nm"]
    assert r["status"]["end"] == serial_flight["status"]["end"]
    assert len(r["groups"]) > 0 and np.array_equal(r["groups"], serial_flight["groups"])


# ---------------------------------------------------------------------------------------------------------------
# 5. larger batches

def _small_against_oracle(pkg, oracle, rows, sizes, key):
    """the unselected path at 130 channels against the oracle: what makes an unselected batch a reference"""
    plan = [{"a": None, "m": None, "pcm": np.float32, "mpx": np.float32}] * len(sizes)
    small = _run(pkg, 130, _shifts(130), rows, sizes, plan)
    _check_against(small, plan, _by_shift(oracle, _shifts(130), rows, key, 0),
                   _by_shift(oracle, _shifts(130), rows, key, 1), "130 unselected channels against the oracle")
    return small


def _random_rows(Cn, n, seed):
    return [int(c) for c in np.random.default_rng(seed).permutation(Cn)[:n]]


def test_selections_of_4160_channels(pkg, oracle, fmsig):
    """4160 channels, calls of 65 536 in flight (whole-CU serial stage, ring resampler beside the writer): random
    selections of 1, 64 and 1000 rows, both outputs, both formats, against the unselected 4160-channel batch -- whose
    path is held against the oracle at 130 channels here, and whose channels equal those by tuner shift."""
    Cn, sizes = 4160, [N, N, N]
    rows = _shared_rows(fmsig, sizes)
    small = _small_against_oracle(pkg, oracle, rows, sizes, "4160")
    fplan = [{"a": None, "m": None, "pcm": np.float32, "mpx": np.float32}] * len(sizes)
    ref = _run(pkg, Cn, _shifts(Cn), rows, sizes, fplan, nbuf=3)
    for k in range(len(sizes)):
        for key in ("a", "m"):
            assert np.array_equal(ref["calls"][k][key].view(np.uint32),
                                  small["calls"][k][key][np.arange(Cn) % 4].view(np.uint32)), (k, key)
    plan = [{"a": _random_rows(Cn, (1, 64, 1000)[k], 10 + k), "m": _random_rows(Cn, (1000, 1, 64)[k], 20 + k),
             "pcm": (np.int16, np.float32, np.int16)[k], "mpx": (np.float32, np.int16, np.float32)[k]}
            for k in range(len(sizes))]
    r = _run(pkg, Cn, _shifts(Cn), rows, sizes, plan, nbuf=3)
    _check_against(r, plan, _of_batch(ref, "a"), _of_batch(ref, "m"), 4160)
    assert r["status"]["end"] == ref["status"]["end"] and np.array_equal(r["groups"], ref["groups"])


def test_selections_of_a_16384_channel_shell(pkg, oracle, fmsig):
    """A shell over two sub-batches, min-size calls: the lists hold global channels, the rows come from both
    sub-batches interleaved in the list, and every sub-batch writes into the one compact output."""
    Cn, sizes = 16384, [8192, 8192, 8192]
    rows = _shared_rows(fmsig, sizes)
    _small_against_oracle(pkg, oracle, rows, sizes, "shell")
    fplan = [{"a": None, "m": None, "pcm": np.float32, "mpx": np.float32}] * len(sizes)
    ref = _run(pkg, Cn, _shifts(Cn), rows, sizes, fplan, nbuf=3)

    def interleaved(n, seed):
        rng = np.random.default_rng(seed)
        lo, hi = rng.permutation(8192)[:(n + 1) // 2], 8192 + rng.permutation(8192)[:n // 2]
        out = np.empty(n, np.int64)
        out[0::2], out[1::2] = lo, hi
        return [int(c) for c in out]

    plan = [{"a": interleaved((1, 64, 1000)[k], 30 + k) + ([8192] if k == 0 else []),
             "m": interleaved((1000, 2, 64)[k], 40 + k), "pcm": (np.int16, np.float32, np.int16)[k],
             "mpx": (np.float32, np.int16, np.float32)[k]} for k in range(len(sizes))]
    for p in plan[1:]:
        assert min(p["a"]) < 8192 <= max(p["a"]) and min(p["m"]) < 8192 <= max(p["m"])
    r = _run(pkg, Cn, _shifts(Cn), rows, sizes, plan, nbuf=3)
    _check_against(r, plan, _of_batch(ref, "a"), _of_batch(ref, "m"), "shell")
    assert r["status"]["end"] == ref["status"]["end"] and np.array_equal(r["groups"], ref["groups"])


# ---------------------------------------------------------------------------------------------------------------
# 6. edits

def test_edited_slots_deliver_the_decoder_they_now_are(pkg, oracle, fmsig):
    """130 channels on two captures, retuning enabled, calls in flight, one selection for both outputs.  In front of
    call 2 a selected and an unselected slot are reset and another pair retuned; in front of call 3 a pair moves to the
    other capture and a pair takes imported decoders of a second batch.  The selected slots' rows are the oracle's for
    the decoder the slot now is; the unselected ones are selected in front of call 4 and deliver theirs from there."""
    Cn, G = 130, 2
    sizes = [N, N, 30001, N, N, N]
    sts = [_station(fmsig, seed=600 + g, pi=0x6100 + g) for g in range(G)]
    rows, start = [], 0
    for n in sizes:
        rows.append(np.stack([fmsig.generate_f32(sts[g], start, n) for g in range(G)]))
        start += n
    shifts, cmap = _shifts(Cn), np.arange(Cn) % G
    first = [5, 7, 9, 11, 4, 129, 64]            # reset, retuned, switched, imported, bystanders
    late = [6, 8, 10, 12]                        # the same edits on slots that deliver nothing until call 4
    src = pkg.Batch(pkg.make_params(FS, -0.15 * FS, 48000.0, 15000.0, D), 2, tuning_shifts=np.array([9, 11], np.int32),
                    record_callbacks=False)      # both on capture 0, fed the same call sizes: the same clock

    def edit(b, k):
        if k == 2:
            b.reset_channels([5, 6])
            b.retune([7, 8], [9, 11])
        if k == 3:
            b.switch_captures([9, 10], [int(1 - cmap[9]), int(1 - cmap[10])])
            b.import_channels([11, 12], src.export_channels([0, 1]))
        src.process_host_fmt(rows[k][0], shared=True)

    plan = [{"a": first if k == 0 else first + late if k == 4 else KEEP,
             "m": first[::-1] if k == 0 else late + first if k == 4 else KEEP,
             "pcm": (np.float32, np.int16)[k % 2], "mpx": (np.int16, np.float32)[k % 2]} for k in range(len(sizes))]
    r = _run(pkg, Cn, shifts, rows, sizes, plan, cmap=cmap, setup=lambda b: b.enable_retune(), edit=edit)
    src.close()

    def decoder_of(c):
        """(audio, tap) per call of the oracle decoder slot c is at that call"""
        sh = {7: 9, 8: 11}.get(c, {11: 9, 12: 11}.get(c, int(shifts[c])))
        o = oracle.OracleDecoder(FS, 0.0, 48000.0, 15000.0, D, tuning_shift=sh)
        old = oracle.OracleDecoder(FS, 0.0, 48000.0, 15000.0, D, tuning_shift=int(shifts[c]))
        out = []
        for k, n in enumerate(sizes):
            cap = int(cmap[c])
            if c in (9, 10) and k >= 3:
                cap = 1 - cap
            if c in (5, 6) and k == 2:
                o.reset()
            if c in (7, 8) and k < 2:      # a decoder of the new shift that heard zeros until the retune
                o.process_stream(np.zeros(2 * n, np.float32))
                out.append((old.process_stream(rows[k][cap]).copy(), old.taps()["baseband"].copy()))
                continue
            if c in (11, 12) and k < 3:    # the imported decoder lived in the source batch, on capture 0
                o.process_stream(rows[k][0])
                out.append((old.process_stream(rows[k][cap]).copy(), old.taps()["baseband"].copy()))
                continue
            out.append((o.process_stream(rows[k][cap]).copy(), o.taps()["baseband"].copy()))
        return out

    dec = {c: decoder_of(c) for c in first + late}
    _check_against(r, plan, lambda k, ch: np.stack([dec[int(c)][k][0] for c in ch]),
                   lambda k, ch: np.stack([dec[int(c)][k][1] for c in ch]), "edits")
    assert [len(s) for s in r["sel_a"]] == [7, 7, 7, 7, 11, 11]


def test_a_loaded_state_leaves_the_selection_alone(pkg, oracle, fmsig):
    """save_state of a batch with one selection, load_state into a batch with another: the destination keeps its own
    selection and delivers the source's bits in those rows; the blob's size per channel is what it was."""
    Cn = 6
    ps = [_station(fmsig, seed=700 + c, pi=0x7700 + c) for c in range(Cn)]
    refs = [oracle.OracleDecoder(FS, -0.15 * FS, 48000.0, 15000.0, D) for _ in range(Cn)]
    mk = lambda: pkg.Batch(pkg.make_params(FS, -0.15 * FS, 48000.0, 15000.0, D), Cn)
    a, b = mk(), mk()
    assert pkg.lib().fmd_batch_state_size(a._h, 2) - pkg.lib().fmd_batch_state_size(a._h, 1) == 8312
    size0 = pkg.lib().fmd_batch_state_size(a._h, Cn)
    a.select_audio([4, 0])
    a.select_mpx([])
    b.select_audio([1, 5, 2])
    b.select_mpx([3])
    assert pkg.lib().fmd_batch_state_size(a._h, Cn) == size0 == pkg.lib().fmd_batch_state_size(b._h, Cn)
    start, want = 0, None
    for k in range(4):
        x = np.stack([fmsig.generate_f32(ps[c], start, N) for c in range(Cn)])
        start += N
        want = [(refs[c].process_stream(x[c]).copy(), refs[c].taps()["baseband"].copy()) for c in range(Cn)]
        if k < 2:
            au, mp = a.process_host_fmt(x, mpx=np.float32)
            assert au.shape[0] == 2 and mp.shape[0] == 0
            _same(au, np.stack([want[4][0], want[0][0]]), pcm16, k)
            b.process_host_fmt(x * np.float32(0.5))  # the destination has a history of its own
            continue
        if k == 2:
            blob = a.save_state()
            assert len(blob) == size0
            b.load_state(blob)
            assert b.audio_selection().tolist() == [1, 5, 2] and b.mpx_selection().tolist() == [3]
            assert a.audio_selection().tolist() == [4, 0] and a.mpx_selection().tolist() == []
        au, mp = b.process_host_fmt(x, pcm=np.int16 if k == 3 else None, mpx=np.int16 if k == 2 else np.float32)
        _same(au, np.stack([want[c][0] for c in (1, 5, 2)]), pcm16, k)
        _same(mp, np.stack([want[3][1]]), mpx16, k)
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. host entry points and the Python layer

def test_host_entry_points_copy_the_selected_rows(pkg, oracle, fmsig):
    """fmd_batch_process_host_mpx / _pcm with selections: n-row arrays of an odd stride behind an unaligned pointer
    hold the selected rows and their fill everywhere else; audio = NULL with an empty audio selection; the multiplex
    with an empty selection is the _pcm call (0 samples, nothing written); Batch.process_host_fmt returns n rows."""
    Cn = 5
    ps = [_station(fmsig, seed=70 + c, **({"dev": 300e3} if c == 1 else {})) for c in range(Cn)]
    refs = [oracle.OracleDecoder(FS, -0.15 * FS, 48000.0, 15000.0, D) for _ in range(Cn)]
    b = pkg.Batch(pkg.make_params(FS, -0.15 * FS, 48000.0, 15000.0, D), Cn)
    lib = pkg.lib()
    start = 0
    cases = [([3, 0, 4], [1]), ([], [4, 2]), ([], []), (None, [0, 1, 2, 3, 4][::-1]), ([1, 3], None), ([2], [])]
    for k, (sa, sm) in enumerate(cases):
        n = (N, 20001, 8192, 33333, N, 8192)[k]
        x = np.stack([fmsig.generate_f32(ps[c], start, n) for c in range(Cn)])
        start += n
        want = [(refs[c].process_stream(x[c]).copy(), refs[c].taps()["baseband"].copy()) for c in range(Cn)]
        b.select_audio(sa)
        b.select_mpx(sm)
        ca = list(range(Cn)) if sa is None else sa
        cm = list(range(Cn)) if sm is None else sm
        if k % 2 == 1:  # the Python layer
            au, mp = b.process_host_fmt(x, pcm=np.int16 if k == 3 else None, mpx=np.int16 if k == 1 else np.float32)
            assert au.shape[0] == len(ca) and mp.shape[0] == len(cm)
            if ca:
                _same(au, np.stack([want[c][0] for c in ca]), pcm16, k)
            if cm:
                _same(mp, np.stack([want[c][1] for c in cm]), mpx16, k)
            else:
                assert mp.size == 0
            continue
        s16a, s16m = k in (2, 4), k == 4
        a_stride, m_stride = b.max_audio_floats(n) + 3, b.max_mpx_samples(n) + 5  # odd
        abuf = np.full((len(ca) + 1) * a_stride + 1, FILL16 if s16a else FILL32, np.int16 if s16a else np.int32)
        mbuf = np.full((len(cm) + 1) * m_stride + 1, FILL16 if s16m else FILL32, np.int16 if s16m else np.int32)
        aout, mout = abuf[1:], mbuf[1:]  # 2- / 4-byte aligned only
        nf, nm = C.c_uint(), C.c_uint(77)
        rc = lib.fmd_batch_process_host_mpx(b._h, x.ctypes.data, pkg.FMD_IQ_F32, n, n,
                                            aout.ctypes.data if ca else None,
                                            pkg.FMD_PCM_S16 if s16a else pkg.FMD_PCM_F32, a_stride, C.byref(nf),
                                            mout.ctypes.data, pkg.FMD_MPX_S16 if s16m else pkg.FMD_MPX_F32, m_stride,
                                            C.byref(nm))
        assert rc >= 0, lib.fmd_last_error()
        assert nf.value == want[0][0].size and nm.value == (want[0][1].size if cm else 0)
        ga, gm = aout.reshape(len(ca) + 1, a_stride), mout.reshape(len(cm) + 1, m_stride)
        if ca:
            got = ga[:len(ca), :nf.value]
            _same(got if s16a else got.view(np.float32), np.stack([want[c][0] for c in ca]), pcm16, k)
        if cm:
            got = gm[:len(cm), :nm.value]
            _same(got if s16m else got.view(np.float32), np.stack([want[c][1] for c in cm]), mpx16, k)
        for g, rows_n, m, fill in ((ga, len(ca), nf.value, FILL16 if s16a else FILL32),
                                   (gm, len(cm), nm.value, FILL16 if s16m else FILL32)):
            assert (g[:rows_n, m:] == fill).all() and (g[rows_n:] == fill).all()
        assert abuf[0] == (FILL16 if s16a else FILL32) and mbuf[0] == (FILL16 if s16m else FILL32)
        if not cm:  # ... the _pcm call: the same audio from it on the next block is checked by the stream going on
            assert nm.value == 0
    # a non-empty audio selection needs the array
    b.select_audio([0])
    x = np.stack([fmsig.generate_f32(ps[c], start, 8192) for c in range(Cn)])
    nf = C.c_uint()
    assert lib.fmd_batch_process_host_pcm(b._h, x.ctypes.data, pkg.FMD_IQ_F32, 8192, 8192, None, pkg.FMD_PCM_F32, 4096,
                                          C.byref(nf)) == -1
    assert b"null" in lib.fmd_last_error()
    au = b.process_host_fmt(x)
    assert au.shape[0] == 1
    _same(au, refs[0].process_stream(x[0])[None, :], pcm16, "after the refusal")
    b.close()


# ---------------------------------------------------------------------------------------------------------------
# 8. refusals on the device box

def test_refusals_leave_the_batch_as_it_was(pkg, oracle, fmsig):
    """Lists the library refuses (a channel twice, out of range, more rows than channels), misaligned S16 rows, a NULL
    d_audio with rows to write and a selection on a decoder's batch (FMD_ERR_STATE): a sentence each, the selection
    and the stream as they were -- the calls in between and behind deliver the oracle's rows, bit for bit."""
    import torch
    Cn = 3
    sizes = [N, 8192, N]
    rows = _shared_rows(fmsig, sizes)
    b = pkg.Batch(pkg.make_params(FS, -0.15 * FS, 48000.0, 15000.0, D), Cn, record_callbacks=False)
    o = oracle.OracleDecoder(FS, -0.15 * FS, 48000.0, 15000.0, D)
    lib = pkg.lib()
    a_stride = (b.max_audio_floats(N) + 7) // 8 * 8
    b.select_audio([2, 0])
    for k, n in enumerate(sizes):
        iq = torch.from_numpy(rows[k]).cuda()
        bad = np.array([1, 1], np.uint32)
        assert lib.fmd_batch_select_audio(b._h, bad.ctypes.data, 2) == -1 and b"listed twice" in lib.fmd_last_error()
        bad = np.array([0, 3], np.uint32)
        assert lib.fmd_batch_select_mpx(b._h, bad.ctypes.data, 2) == -1 and b"out of range" in lib.fmd_last_error()
        bad = np.array([0, 1, 2, 0], np.uint32)
        assert lib.fmd_batch_select_audio(b._h, bad.ctypes.data, 4) == -1 and b"more rows" in lib.fmd_last_error()
        assert b.audio_selection().tolist() == [2, 0] and b.mpx_selection().tolist() == [0, 1, 2]
        s16 = k == 1
        out = _Rows(Cn, a_stride, s16)
        with pytest.raises(pkg.FmdError, match="fmd error -1: .*null argument"):
            b.process_device(iq.data_ptr(), 0, n, None, a_stride, pcm=np.int16 if s16 else np.float32)
        if s16:
            with pytest.raises(pkg.FmdError, match="fmd error -1: .*16-byte aligned"):
                b.process_device(iq.data_ptr(), 0, n, out.ptr() + 4, a_stride, pcm=np.int16)
            with pytest.raises(pkg.FmdError, match="fmd error -1: .*multiple of 8"):
                b.process_device(iq.data_ptr(), 0, n, out.ptr(), a_stride + 4, pcm=np.int16)
        assert out.host(0, 0)[1]  # nothing was written
        nf = b.process_device(iq.data_ptr(), 0, n, out.ptr(), a_stride, pcm=np.int16 if s16 else np.float32)
        torch.cuda.synchronize()
        got, clean = out.host(2, nf)
        want = o.process_stream(rows[k][0])
        assert clean
        _same(got, np.stack([want, want]), pcm16, k)
    b.close()
    d = pkg.FmDecoder(FS, -0.15 * FS, 48000.0, 15000.0, D)
    view = d.batch_view()
    one = np.zeros(1, np.uint32)
    for fn in (lib.fmd_batch_select_audio, lib.fmd_batch_select_mpx):
        assert fn(view._h, one.ctypes.data, 1) == -4, lib.fmd_last_error()  # FMD_ERR_STATE
        assert b"fmd_decoder" in lib.fmd_last_error()
    assert view.audio_selection().tolist() == [0]
    o = oracle.OracleDecoder(FS, -0.15 * FS, 48000.0, 15000.0, D)
    for k in range(2):
        assert np.array_equal(d.ProcessStream(rows[k][0].view(np.complex64)).view(np.uint32),
                              o.process_stream(rows[k][0]).view(np.uint32))
    d.close()
