"""Channel IQ rows as the INPUT of a call (FMD_IN_CIQ_*, the call record of include/fmd.h): the IF stage does not run,
k_ciq_in copies the caller's rows -- float pairs, or pairs of 16-bit integers times 2^-13 -- into the rows that stage
would have written, and everything behind it decodes them as the output of a call of baseband length M.

The contract needs no tolerance.  A call that is fed the CPU oracle's `demod` tap of a block (m_BufferIF behind
cDownsampleFilter::Process) has to deliver what the oracle delivers for that block: audio (float: the bits; int16:
pcm16 of them), the multiplex (the oracle's baseband tap), the channel IQ out (the input's bits), the feed (the
definition of tests/feed_spec.py over the oracle's audio), the status record without interface_level (the one field
that reads raw IQ) and the RDS groups.  Where a batch is beyond the oracle's reach the expected values are those of the
channel of the same tuner shift in a small batch held against the oracle in the same test; never the output under test.
Input rows are padded with NaN behind their M samples and output rows pre-filled: nothing behind M is read or written.
Every comparison is an equality, NaN for NaN."""
import ctypes as C

import numpy as np
import pytest

import feed_spec
from __graft_entry__ import load_package
from feed_spec import mpx16

pytestmark = pytest.mark.gpu

FS, D, N = 2.4e6, 11, 65536
RAGGED = [88, 89, 97, 100, 150, 170, 301, 1001, 3663, 8191, 12345, 40000]  # M = 8 (the smallest) .. 3636, M % 4 all
PURE = [N] * 5 + RAGGED + [30001, N, N]
FILL = 77.0
M_STRIDE = 5968


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def pcm16(x):
    y = np.asarray(x, np.float32) * np.float32(32768.0)
    with np.errstate(invalid="ignore"):
        r = np.clip(np.rint(y), -32768.0, 32767.0)
    return np.where(np.isnan(y), 0, r).astype(np.int16)


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _shifts(Cn):
    return [(10, 9, 10, 11)[c % 4] for c in range(Cn)]


def _to_s16(rows):
    """complex64 [.., M] -> int16 [.., M, 2]: FMD_CIQ_S16 of the rows (what an archive of 16-bit rows holds)"""
    return np.stack([mpx16(rows.real), mpx16(rows.imag)], axis=-1)


def _from_s16(rows):
    """int16 [.., M, 2] -> complex64 [.., M]: the host's conversion, (float)v * 2^-13"""
    f = rows.astype(np.float32) * np.float32(2.0 ** -13)
    return np.ascontiguousarray(f).view(np.complex64)[..., 0]


_REF = {}


def _reference(oracle, fmsig, key, sizes, shifts, fs=FS, Dv=D, **station):
    """(the blocks of one station, per tuner shift the oracle's record of every call), computed once per stream"""
    need = sorted(set(int(s) for s in shifts))
    if key not in _REF:
        p, blocks, start = fmsig.default_params(fs, noise_sigma=0.005, **station), [], 0
        for n in sizes:
            blocks.append(fmsig.generate_f32(p, start, n))
            start += n
        _REF[key] = (blocks, {})
    blocks, per = _REF[key]
    for s in need:
        if s in per:
            continue
        o = oracle.OracleDecoder(fs, 0.0, 48000.0, 15000.0, Dv, tuning_shift=s)
        calls, ng = [], 0
        for x in blocks:
            audio = o.process_stream(x)
            t, g = o.taps(), o.rds_groups(ng)
            ng += len(g)
            calls.append({"demod": t["demod"], "mpx": t["baseband"], "audio": audio, "status": o.status(),
                          "groups": [blk for _, blk in g]})
        o.close()
        per[s] = calls
    return blocks, per


def _rows_of(per, shifts, k, what="demod"):
    return np.stack([per[int(s)][k][what] for s in shifts])


def _status_words(s, oracle_side):
    """the status record without interface_level, floats as their bits"""
    f = (s.tuning_offset, s.baseband_level, s.pilot_level)
    return (bool(s.stereo if oracle_side else s.stereo_detected), int(s.rds_state)) + tuple(
        int(np.float32(v).view(np.uint32)) for v in f)


def _run(pkg, Cn, shifts, calls, fs=FS, Dv=D, mode=2, lag=2, setup=None, feed=0, blocks=0, status_at=(), profiling=0):
    """One batch, device buffers of its own for every call, calls submitted back to back (concurrency 2: the outputs are
    waited for `lag` calls late, and read at the end).  calls[k]: {"iq": float32 [2 n], one shared capture} or {"ciq":
    complex64 [Cn, M] / int16 [Cn, M, 2] rows}; "pcm": the audio format.  Returns per call the audio, multiplex, channel IQ out and feed rows with their counts and whether every
    row was untouched behind them; the status words at the end (and behind the calls of status_at), the groups per
    channel, the block records."""
    import torch
    b = pkg.Batch(pkg.make_params(fs, -0.15 * fs, 48000.0, 15000.0, Dv), Cn, tuning_shifts=np.array(shifts, np.int32),
                  record_callbacks=False)
    b.set_concurrency(mode)
    if setup:
        setup(b)
    if feed:
        b.set_feed(feed)
    if blocks:
        b.set_rds_blocks(blocks, 1 << 16)
    if profiling:
        b.set_profiling(profiling)
    st = torch.cuda.current_stream().cuda_stream
    a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
    f_stride = (max(b.max_feed_samples(N), 1) + 8) // 8 * 8
    keep, res, status = [], [], {}
    for k, c in enumerate(calls):
        s16 = np.dtype(c.get("pcm", np.float32)) == np.int16
        out = {"audio": torch.zeros((Cn, a_stride), dtype=torch.int16 if s16 else torch.float32, device="cuda"),
               "mpx": torch.full((Cn, M_STRIDE), FILL, dtype=torch.float32, device="cuda"),
               "ciq": torch.full((Cn, 2 * M_STRIDE), FILL, dtype=torch.float32, device="cuda"),
               "feed": torch.full((Cn, f_stride), FILL, dtype=torch.float32, device="cuda")}
        n = {name: C.c_uint(12345) for name in out}
        rows = dict(audio=pkg.make_rows(out["audio"].data_ptr(), pkg.FMD_PCM_S16 if s16 else pkg.FMD_PCM_F32, a_stride,
                                        n["audio"]),
                    mpx=pkg.make_rows(out["mpx"].data_ptr(), pkg.FMD_MPX_F32, M_STRIDE, n["mpx"]),
                    ciq=pkg.make_rows(out["ciq"].data_ptr(), pkg.FMD_CIQ_F32, M_STRIDE, n["ciq"]), stream=st)
        if feed:
            rows["feed"] = pkg.make_rows(out["feed"].data_ptr(), pkg.FMD_FEED_F32, f_stride, n["feed"])
        if "ciq" in c:
            x = np.ascontiguousarray(c["ciq"])
            m = x.shape[1]
            if x.dtype == np.int16:  # rows padded to a stride of 4 samples with a value that would show
                pad = np.full((Cn, (m + 3) // 4 * 4 + 4, 2), 0x7A7A, np.int16)
            else:  # ... of 2 samples, with NaN
                assert x.dtype == np.complex64
                pad = np.full((Cn, (m + 1) // 2 * 2 + 2), np.nan + 1j * np.nan, np.complex64)
            pad[:, :m] = x
            t = torch.from_numpy(pad).cuda()
            b.process_call(ciq_in=t[:, :m], **rows)
        else:
            t = torch.from_numpy(np.ascontiguousarray(c["iq"])).cuda()
            b.process_call(pkg.make_call(t.data_ptr(), pkg.FMD_IQ_F32, 0, c["iq"].size // 2, **rows))
        keep.append(t)
        res.append((out, n))
        if k in status_at:
            b.wait(stream=st)
            torch.cuda.synchronize()
            status[k] = [(_status_words(b.status(ch), False), b.status(ch).interface_level) for ch in range(Cn)]
        elif mode == 2 and k >= lag:
            b.wait(stream=st, lag=lag)
        elif mode != 2:
            b.wait(stream=st)
    b.wait(stream=st)
    torch.cuda.synchronize()
    final = []
    for out, n in res:
        r = {"n": {name: v.value for name, v in n.items()}, "clean": True}
        for name, width in (("audio", 1), ("mpx", 1), ("ciq", 2), ("feed", 1)):
            if name == "feed" and not feed:
                continue
            a = out[name].cpu().numpy()
            cnt = r["n"][name] * width
            r[name] = a[:, :cnt].copy()
            if name != "audio":
                r["clean"] = r["clean"] and bool((a[:, cnt:] == np.float32(FILL)).all())
        r["ciq"] = np.ascontiguousarray(r["ciq"]).view(np.complex64)
        final.append(r)
    step = max(1, Cn // 64)
    status["end"] = {ch: (_status_words(b.status(ch), False), b.status(ch).interface_level)
                     for ch in range(0, Cn, step)}
    g = np.sort(b.collect_rds_array(cap=1 << 18, stream=st), order=["channel", "call_index"])
    groups = {ch: [(int(ci), tuple(int(v) for v in blk)) for c_, ci, blk in zip(g["channel"], g["call_index"],
                                                                              g["blocks"]) if int(c_) == ch]
              for ch in range(0, Cn, step)}
    recs = b.collect_rds_blocks(cap=1 << 18)[0] if blocks == 2 else None
    quality = b.rds_quality().copy() if blocks else None
    limits = b.baseband_limits()
    stage_ms = b.stage_ms() if profiling else None
    b.close()
    return {"stage_ms": stage_ms, "calls": final, "status": status, "groups": groups, "blocks": recs, "quality": quality, "limits": limits}


def _check_against_oracle(r, per, shifts, calls, taps, what):
    """every call's outputs, the end status and the groups of a run against the oracle's records of the same calls"""
    Cn = len(shifts)
    spec = feed_spec.FeedSpec(taps, 2, Cn) if taps is not None else None
    for k, c in enumerate(calls):
        got, s16 = r["calls"][k], np.dtype(c.get("pcm", np.float32)) == np.int16
        audio = _rows_of(per, shifts, k, "audio")
        assert got["clean"], (what, k)
        assert _bits(got["audio"], pcm16(audio) if s16 else audio), (what, "audio", k)
        assert _bits(got["mpx"], _rows_of(per, shifts, k, "mpx")), (what, "mpx", k)
        assert _bits(got["ciq"], _rows_of(per, shifts, k, "demod")), (what, "ciq out", k)
        assert got["n"]["ciq"] == got["n"]["mpx"] == per[int(shifts[0])][k]["demod"].size
        if spec is not None:
            assert _bits(got["feed"], spec.push(audio)), (what, "feed", k)
    for ch, (words, _) in r["status"]["end"].items():
        assert words == _status_words(per[int(shifts[ch])][-1]["status"], True), (what, "status", ch)
    n_groups = 0
    for ch, got in r["groups"].items():
        want = [(k + 1, blk) for k in range(len(calls)) for blk in per[int(shifts[ch])][k]["groups"]]
        assert got == want, (what, "groups", ch)
        n_groups += len(want)
    return n_groups


# ---------------------------------------------------------------------------------------------------------------
# 1. pure: every call brings its baseband

@pytest.mark.parametrize("Cn", [1, 63, 65, 130])
def test_pure_channel_iq_batch_equals_the_oracle(pkg, oracle, fmsig, Cn):
    """Batches that end inside a wave, at a wave and one channel behind it, tuner shifts 9 / 10 / 11 mixed on one
    capture; twenty calls, twelve of them ragged down to M = 8, the smallest this geometry accepts (fmd_batch_
    baseband_limits), with M = 0, 1, 2, 3 mod 4 -- the partial groups of k_ciq_in; each call is fed the oracle's demod
    tap of the block.  Audio in both formats, multiplex, channel IQ out, feed, status without interface_level and the
    RDS groups are the oracle's; interface_level stays what a batch that never saw IQ has.  63 channels: with block
    records, which are those of a batch fed the IQ itself."""
    shifts = _shifts(Cn)
    blocks, per = _reference(oracle, fmsig, "pure", PURE, shifts)
    ms = [per[10][k]["demod"].size for k in range(len(PURE))]
    assert min(ms) == 8 and {m % 4 for m in ms} == {0, 1, 2, 3}
    calls = [{"ciq": _rows_of(per, shifts, k), "pcm": np.int16 if k % 2 else np.float32} for k in range(len(PURE))]
    taps = None

    def setup(b):
        nonlocal taps
        b.set_feed(2)
        taps = b.feed_taps()

    rb = 2 if Cn == 63 else 0
    r = _run(pkg, Cn, shifts, calls, setup=setup, feed=2, blocks=rb)
    assert r["limits"] == (8, 5958, 1)
    assert _check_against_oracle(r, per, shifts, calls, taps, ("pure", Cn)) > 0
    assert all(level == 0.0 for _, level in r["status"]["end"].values())  # no level meter ever ran
    if rb:
        iq = [{"iq": blocks[k], "pcm": calls[k]["pcm"]} for k in range(len(PURE))]
        want = _run(pkg, Cn, shifts, iq, feed=2, blocks=rb)
        assert len(want["blocks"]) > 100 and _bits(r["blocks"], want["blocks"])
        assert _bits(r["quality"], want["quality"])


@pytest.mark.parametrize("fs,Dv,sizes", [(2.4e6, 11, [N, 30001, 88, N]), (6.4e6, 1, [32000, 20000, 4000, 32000])],
                         ids=["2p4M-D11", "6p4M-D1-cic"])
def test_single_decoder(pkg, oracle, fmsig, fs, Dv, sizes):
    """fmd_process_stream_call through FmDecoder.ProcessChannelIq (host rows, no stride, any alignment): audio as float
    and int16 and the multiplex are the oracle's, from float rows and from 16-bit rows; with CIC stages in front of the
    RDS decimator an odd M is refused with the plan's sentence and leaves the decoder as it was."""
    p = fmsig.default_params(fs, noise_sigma=0.005)
    o = oracle.OracleDecoder(fs, -0.15 * fs, 48000.0, 15000.0, Dv)
    d32, d16, dm = (pkg.FmDecoder(fs, -0.15 * fs, 48000.0, 15000.0, Dv) for _ in range(3))
    lo, hi, mult = d32.batch_view().baseband_limits()
    assert mult == (2 if Dv == 1 else 1) and hi == (N + Dv - 1) // Dv
    start = 0
    for k, n in enumerate(sizes):
        ref = o.process_stream(fmsig.generate_f32(p, start, n))
        start += n
        tap, mpx = o.taps()["demod"], o.taps()["baseband"]
        if mult == 2:
            with pytest.raises(pkg.FmdError, match="fmd error -3: .*CIC"):
                d32.ProcessChannelIq(tap[:tap.size - 1])
        raw = np.zeros(2 * tap.size + 1, np.float32)  # (a pointer on no 8-byte boundary)
        raw[1:] = tap.view(np.float32)
        assert _bits(d32.ProcessChannelIq(raw[1:].view(np.complex64)), ref), k
        assert _bits(d16.ProcessChannelIq(tap, pcm=np.int16), pcm16(ref)), k
        a, m = dm.ProcessChannelIq(tap, mpx=np.float32)
        assert _bits(a, ref) and _bits(m, mpx), k
    assert d32.StereoDetected() == bool(o.status().stereo)
    for d in (d32, d16, dm):
        assert d.GetInterfaceLevel() == 0.0
        assert np.float32(d.GetPilotLevel()) == np.float32(o.status().pilot_level)


@pytest.mark.parametrize("level,mode", [(1, 2), (2, 2), (1, 1)])
def test_profiled_calls_report_the_copy_in_the_if_stages_slot(pkg, oracle, fmsig, level, mode):
    """Profiling levels 1 (the IF kernel's own start and stop) and 2 (events between all stages, calls in order): the
    outputs stay the oracle's, and the stage-time getter reports the copying kernel where it reports the IF FIR."""
    Cn, sizes = 65, [N, 12345, N]
    shifts = _shifts(Cn)
    _, per = _reference(oracle, fmsig, "poison", sizes, shifts)
    calls = [{"ciq": _rows_of(per, shifts, k)} for k in range(len(sizes))]
    r = _run(pkg, Cn, shifts, calls, mode=mode, profiling=level)
    _check_against_oracle(r, per, shifts, calls, None, ("profiling", level))
    stages, n_calls = r["stage_ms"]
    first = next(iter(stages.items()))
    print("level %d, concurrency %d: %s = %.4f ms over %d calls" % (level, mode, first[0], first[1], n_calls))
    assert n_calls == len(sizes) and 0.0 < first[1] < 5.0


# ---------------------------------------------------------------------------------------------------------------
# 2. 16-bit rows

def test_s16_rows_equal_the_float_call_on_converted_rows(pkg, oracle, fmsig):
    """Device calls with int16 rows (an archive made with FMD_CIQ_S16: mpx16 of the oracle's tap) against device calls
    with the float rows the host converts them to, (float)v * 2^-13: every output has the same bits.  Then the host call
    with both, the 16-bit rows at an odd stride from a pointer on no 4-byte boundary."""
    Cn, sizes = 65, [N, 8191, 97, 12345, N]
    shifts = _shifts(Cn)
    _, per = _reference(oracle, fmsig, "s16", sizes, shifts)
    q = [_to_s16(_rows_of(per, shifts, k)) for k in range(len(sizes))]
    r16 = _run(pkg, Cn, shifts, [{"ciq": x} for x in q])
    r32 = _run(pkg, Cn, shifts, [{"ciq": _from_s16(x)} for x in q])
    for k in range(len(sizes)):
        assert r16["calls"][k]["clean"] and r16["calls"][k]["n"] == r32["calls"][k]["n"]
        for name in ("audio", "mpx", "ciq"):
            assert _bits(r16["calls"][k][name], r32["calls"][k][name]), (name, k)
        assert _bits(r16["calls"][k]["ciq"], _from_s16(q[k])), k  # the channel IQ out: the converted input, as floats
        assert float(np.abs(r16["calls"][k]["audio"]).max()) > 0.01  # (not silence)
    assert r16["status"]["end"] == r32["status"]["end"] and r16["groups"] == r32["groups"]
    # host calls: any stride >= M, any alignment
    b16, b32 = (pkg.Batch(pkg.make_params(FS, -0.15 * FS, 48000.0, 15000.0, D), Cn,
                          tuning_shifts=np.array(shifts, np.int32), record_callbacks=False) for _ in range(2))
    for k in range(len(sizes)):
        m = q[k].shape[1]
        raw = np.zeros(2 * (Cn * (m + 3) * 2 + 1), np.uint8)
        odd = raw[2:].view(np.int16).reshape(Cn, m + 3, 2)  # (rows 4 m + 12 bytes apart, from base + 2)
        odd[:, :m] = q[k]
        odd[:, m:] = 0x7A7A
        a16, m16, c16 = b16.process_host_ciq_in(odd[:, :m], mpx=np.float32, ciq=np.complex64)
        a32, m32, c32 = b32.process_host_ciq_in(_from_s16(q[k]), mpx=np.float32, ciq=np.complex64)
        assert _bits(a16, a32) and _bits(m16, m32) and _bits(c16, c32), k
        assert _bits(a16, r32["calls"][k]["audio"]) and _bits(c16, _from_s16(q[k])), k
    b16.close()
    b32.close()


# ---------------------------------------------------------------------------------------------------------------
# 3. mixed: IQ calls and channel IQ calls in one stream

_MIXED = [32768, 8193, 30001, 12345, 16384] * 4


def _mixed_reference(oracle, fmsig, shifts):
    """One capture cut into 20 blocks.  The even blocks go in as IQ calls; the odd ones come back as channel IQ rows from
    ANOTHER stream: an oracle that decoded the whole capture, whose IF stage saw every block.  The batch's IF stage
    sees the even blocks alone, so its rows must be the demod taps of a second oracle that decoded only those -- rows
    that differ from the first oracle's in the filter's history at the head of every block.  Per shift: the rows every
    call puts behind the IF stage, and the second oracle's interface level."""
    key = "mixed"
    if key not in _REF:
        p, blocks, start = fmsig.default_params(FS, noise_sigma=0.005), [], 0
        for n in _MIXED:
            blocks.append(fmsig.generate_f32(p, start, n))
            start += n
        _REF[key] = (blocks, {})
    blocks, per = _REF[key]
    for s in sorted(set(shifts)):
        if s in per:
            continue
        alone = oracle.OracleDecoder(FS, 0.0, 48000.0, 15000.0, D, tuning_shift=s)
        whole = oracle.OracleDecoder(FS, 0.0, 48000.0, 15000.0, D, tuning_shift=s)
        demod = []
        for k, x in enumerate(blocks):
            whole.process_stream(x)
            if k % 2 == 0:
                alone.process_stream(x)
                demod.append(alone.taps()["demod"])
                assert k == 0 or not _bits(demod[-1], whole.taps()["demod"])  # (the two streams do differ)
            else:
                demod.append(whole.taps()["demod"])
        level = alone.status().if_level
        alone.close()
        whole.close()
        per[s] = {"demod": demod, "if_level": level}
    return blocks[0::2], per


_PURE_OF_MIXED = {}


@pytest.mark.parametrize("how,mode,lag", [(h, 2, g) for h in ("default", "split_post", "lpf_late0", "lpf_late1",
                                                               "lpf_late2") for g in (1, 2, 3)]
                         + [("default", 0, 0), ("default", 1, 0)])
def test_iq_and_channel_iq_calls_in_one_stream(pkg, oracle, fmsig, how, mode, lag):
    """130 channels, 20 calls in flight, IQ calls of one station alternating with channel-IQ calls that bring the
    baseband of another (float and 16-bit rows in turn), on every stream layout and in every concurrency mode.
    The IF stage's state is untouched by the calls between: every IQ call's channel IQ out is the oracle's demod tap
    for a stream of the IQ blocks ALONE.  Downstream the calls are one sequence: audio, multiplex, status and groups
    equal those of a pure channel-IQ batch fed the concatenated rows (which test 1 holds against the oracle).
    interface_level is the oracle's for the IQ blocks alone, unchanged across a channel-IQ call."""
    Cn = 130
    shifts = _shifts(Cn)
    a, per = _mixed_reference(oracle, fmsig, shifts)
    rows = [np.stack([per[s]["demod"][k] for s in shifts]) for k in range(len(_MIXED))]
    # (16-bit rows: the values an archive holds -- downstream sees their conversion)
    fed = [rows[k] if k % 4 != 3 else _from_s16(_to_s16(rows[k])) for k in range(len(_MIXED))]
    calls = [{"iq": a[k // 2]} if k % 2 == 0 else {"ciq": rows[k] if k % 4 != 3 else _to_s16(rows[k])}
             for k in range(len(_MIXED))]
    for k, c in enumerate(calls):
        c["pcm"] = np.int16 if k % 3 == 1 else np.float32
    setup = {"default": None, "split_post": lambda b: b.debug_set("split_post", 1),
             "lpf_late0": lambda b: b.debug_set("lpf_late", 0), "lpf_late1": lambda b: b.debug_set("lpf_late", 1),
             "lpf_late2": lambda b: b.debug_set("lpf_late", 2)}[how]
    r = _run(pkg, Cn, shifts, calls, mode=mode, lag=lag, setup=setup, status_at=(16, 17))
    if "pure" not in _PURE_OF_MIXED:
        _PURE_OF_MIXED["pure"] = _run(pkg, Cn, shifts, [{"ciq": fed[k], "pcm": calls[k]["pcm"]}
                                                       for k in range(len(_MIXED))], mode=1)
    want = _PURE_OF_MIXED["pure"]
    for k in range(len(_MIXED)):
        got = r["calls"][k]
        assert got["clean"] and got["n"] == want["calls"][k]["n"], k
        assert _bits(got["ciq"], fed[k]), ("the rows behind the IF stage", how, mode, lag, k)
        for name in ("audio", "mpx"):
            assert _bits(got[name], want["calls"][k][name]), (name, how, mode, lag, k)
    assert len(want["groups"][0]) + len(want["groups"][2]) > 0
    assert r["groups"] == want["groups"]
    for ch in r["status"]["end"]:
        assert r["status"]["end"][ch][0] == want["status"]["end"][ch][0], ch
    # the level meter: the IQ call 16's value, still there behind the channel-IQ call 17, and at the end (call 18
    # was the last IQ call) the oracle's for the IQ blocks alone
    assert [lv for _, lv in r["status"][16]] == [lv for _, lv in r["status"][17]]
    assert all(lv > 0.0 for _, lv in r["status"][16])
    for ch, (_, lv) in r["status"]["end"].items():
        assert np.float32(lv) == np.float32(per[shifts[ch]]["if_level"]), ch


# ---------------------------------------------------------------------------------------------------------------
# 4. large batches

def test_scale_4160_channels_and_a_shell_of_16384(pkg, oracle, fmsig):
    """4160 channels (the whole-CU serial stage, the half-band chain without mixed rows) and 16 384 (two sub-batches:
    every sub-batch reads its own rows of the one input), three calls in flight: every sampled channel's outputs equal
    those of the channel of the same tuner shift in a 130-channel batch, which is held against the oracle here."""
    sizes = [16384] * 3
    small_shifts = _shifts(130)
    _, per = _reference(oracle, fmsig, "scale", sizes, small_shifts)
    small_calls = [{"ciq": _rows_of(per, small_shifts, k)} for k in range(3)]
    small = _run(pkg, 130, small_shifts, small_calls)
    _check_against_oracle(small, per, small_shifts, small_calls, None, "130 channels")
    for Cn in (4160, 16384):
        shifts = _shifts(Cn)
        r = _run(pkg, Cn, shifts, [{"ciq": _rows_of(per, shifts, k), "pcm": np.int16 if k == 1 else np.float32}
                                   for k in range(3)])
        for k in range(3):
            got = r["calls"][k]
            assert got["clean"], (Cn, k)
            audio = _rows_of(per, shifts, k, "audio")
            assert _bits(got["audio"], pcm16(audio) if k == 1 else audio), (Cn, k)
            assert _bits(got["mpx"], _rows_of(per, shifts, k, "mpx")), (Cn, k)
            assert _bits(got["ciq"], _rows_of(per, shifts, k)), (Cn, k)
        for ch, (words, _) in r["status"]["end"].items():
            assert words == _status_words(per[shifts[ch]][-1]["status"], True), (Cn, ch)


# ---------------------------------------------------------------------------------------------------------------
# 5. refusals that need a batch, and what they leave

def test_refusals_leave_the_batch_as_it_was(pkg, oracle, fmsig):
    """M outside fmd_batch_baseband_limits, a row stride below M, a misaligned device pointer: FMD_ERR_SIZE / _ARG with
    a sentence, nothing submitted; positional entry points refuse the formats on a live batch too.  The calls around
    the refusals decode like an uninterrupted stream."""
    import torch
    Cn, sizes = 2, [N, 8191, N]
    shifts = [10, 9]
    _, per = _reference(oracle, fmsig, "refuse", sizes, shifts)
    b = pkg.Batch(pkg.make_params(FS, -0.15 * FS, 48000.0, 15000.0, D), Cn, tuning_shifts=np.array(shifts, np.int32),
                  record_callbacks=False)
    lo, hi, mult = b.baseband_limits()
    assert (lo, hi, mult) == (b.min_samples() // D, b.max_mpx_samples(N), 1)
    a_stride = (b.max_audio_floats(N) + 7) // 8 * 8
    audio = torch.zeros((Cn, a_stride), dtype=torch.float32, device="cuda")
    big = torch.zeros((Cn, 6000), dtype=torch.complex64, device="cuda")
    out = pkg.make_rows(audio.data_ptr(), pkg.FMD_PCM_F32, a_stride)
    for k in range(len(sizes)):
        with pytest.raises(pkg.FmdError, match="fmd error -3: .*fmd_batch_baseband_limits"):
            b.process_call(ciq_in=big[:, :hi + 1], audio=out)
        with pytest.raises(pkg.FmdError, match="fmd error -3: "):
            b.process_call(ciq_in=big[:, :lo - 1], audio=out)
        with pytest.raises(pkg.FmdError, match="fmd error -1: .*at least samples"):
            b.process_call(pkg.make_call(big.data_ptr(), pkg.FMD_IN_CIQ_F32, 1000, 1002, audio=out))
        with pytest.raises(pkg.FmdError, match="fmd error -1: .*16-byte aligned"):
            b.process_call(pkg.make_call(big.data_ptr() + 8, pkg.FMD_IN_CIQ_F32, 6000, 1000, audio=out))
        with pytest.raises(pkg.FmdError, match="fmd error -1: .*_call entry points only"):
            b.process_device(big.data_ptr(), 6000, 1000, audio.data_ptr(), a_stride, fmt=pkg.FMD_IN_CIQ_F32, pcm=np.float32)
        rows = _rows_of(per, shifts, k)
        got = b.process_host_ciq_in(rows)
        assert _bits(got, _rows_of(per, shifts, k, "audio")), k
        assert _bits(b.tap("demod", 1), rows[1]), k  # the debug tap behind such a call returns the row
    b.close()


# ---------------------------------------------------------------------------------------------------------------
# 6. poison

@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_a_poisoned_row_stays_in_its_channel(pkg, oracle, fmsig, value):
    """65 channels, channel 7's rows hold a NaN / an infinity from the second call on: every other channel's outputs
    keep the oracle's bits and the channel IQ out returns the poison bit for bit.  A NaN reaches channel 7's audio (the
    FM PLL's arctangent and every filter behind it carry it on); an infinity need not: the arctangent of an infinite
    part is finite."""
    Cn, sizes = 65, [N, 12345, N]
    shifts = _shifts(Cn)
    _, per = _reference(oracle, fmsig, "poison", sizes, shifts)
    calls = []
    for k in range(len(sizes)):
        rows = _rows_of(per, shifts, k).copy()
        if k >= 1:
            rows[7, 5] = np.complex64(complex(value, 0.25))
        calls.append({"ciq": rows})
    r = _run(pkg, Cn, shifts, calls)
    others = [c for c in range(Cn) if c != 7]
    for k in range(len(sizes)):
        got = r["calls"][k]
        assert _bits(got["audio"][others], _rows_of(per, shifts, k, "audio")[others]), k
        assert _bits(got["mpx"][others], _rows_of(per, shifts, k, "mpx")[others]), k
        assert _bits(got["ciq"], calls[k]["ciq"]), k  # the channel IQ out is the input, NaN for NaN
    if np.isnan(value):
        assert np.isnan(r["calls"][2]["audio"][7]).any()
    assert _bits(r["calls"][0]["audio"][7], per[shifts[7]][0]["audio"])


# ---------------------------------------------------------------------------------------------------------------
# 7. edits and state between such calls

def test_edits_and_state_between_channel_iq_calls(pkg, oracle, fmsig):
    """Five channels behind a capture map, host calls.  In front of call 1 channel 1 is reset: fed the demod taps of an
    oracle decoder that was Reset() there, it delivers that decoder's audio.  In front of call 2 channel 3 becomes a
    copy of channel 0 (export / import) and, fed channel 0's rows, delivers channel 0's audio; channel 4 is retuned: it
    then is a decoder that received zeros until now, and fed the taps of an oracle that did, delivers that oracle's
    audio.  In front of call 3 the batch is saved and loaded into a second one, which from there on delivers the same
    bits; in front of call 4 channel 2 switches captures, which a call that consults no map does not notice."""
    Cn, sizes = 5, [N, 30001, N, 20001, N]
    shifts = [10, 10, 9, 11, 9]
    blocks, per = _reference(oracle, fmsig, "edits", sizes, shifts)

    def oracle_of(shift, feed, reset_at=None):
        o, out = oracle.OracleDecoder(FS, 0.0, 48000.0, 15000.0, D, tuning_shift=shift), []
        for k, x in enumerate(feed):
            if k == reset_at:
                o.reset()
            audio = o.process_stream(x)
            out.append({"demod": o.taps()["demod"], "audio": audio})
        o.close()
        return out

    was_reset = oracle_of(10, blocks, reset_at=1)
    was_silent = oracle_of(9, [np.zeros_like(x) if k < 2 else x for k, x in enumerate(blocks)])
    source = [[per[10][k] for k in range(5)],
              [per[10][0]] + was_reset[1:],
              [per[9][k] for k in range(5)],
              [per[11][0], per[11][1]] + [per[10][k] for k in range(2, 5)],
              [per[9][0], per[9][1]] + was_silent[2:]]

    def mk():
        b = pkg.Batch(pkg.make_params(FS, -0.15 * FS, 48000.0, 15000.0, D), Cn,
                      tuning_shifts=np.array(shifts, np.int32), record_callbacks=False)
        b.enable_retune()
        b.set_capture_map([0] * Cn, 2)
        return b

    b, b2 = mk(), mk()
    for k in range(len(sizes)):
        if k == 1:
            b.reset_channels([1])
        if k == 2:
            b.import_channels([3], b.export_channels([0]))
            b.retune([4], [9])
        if k == 3:
            b2.load_state(b.save_state())
        if k == 4:
            b.switch_captures([2], [1])
            b2.switch_captures([2], [1])
        rows = np.stack([source[c][k]["demod"] for c in range(Cn)])
        got = b.process_host_ciq_in(rows)
        for c in range(Cn):
            assert _bits(got[c], source[c][k]["audio"]), (k, c)
        if k >= 3:
            assert _bits(b2.process_host_ciq_in(rows), got), ("loaded batch", k)
    assert _bits(b.tap("demod", 4), source[4][4]["demod"])  # the debug tap behind such a call returns the row
    b.close()
    b2.close()


# ---------------------------------------------------------------------------------------------------------------
# 8. teeth

def test_a_skipped_tile_of_the_copy_fails_the_pure_check(pkg, oracle, fmsig):
    """fmd_batch_debug_ciq_in_skip_tile leaves every row's last tile of 512 samples out of the copy: the pure check of
    test 1 has to fail at the first call, in the channel IQ out and in the audio."""
    Cn = 65
    shifts = _shifts(Cn)
    _, per = _reference(oracle, fmsig, "pure", PURE, shifts)
    calls = [{"ciq": _rows_of(per, shifts, k)} for k in range(3)]
    r = _run(pkg, Cn, shifts, calls, setup=lambda b: b.debug_ciq_in_skip_tile(True))
    with pytest.raises(AssertionError):
        _check_against_oracle(r, per, shifts, calls, None, "mutant")
    got = r["calls"][0]
    m = got["n"]["ciq"]
    tile = (m - 1) // 512 * 512
    assert _bits(got["ciq"][:, :tile], calls[0]["ciq"][:, :tile])  # the tiles that were copied
    assert not _bits(got["ciq"][:, tile:], calls[0]["ciq"][:, tile:])
    assert not _bits(got["audio"], _rows_of(per, shifts, 0, "audio"))
