"""Non-finite, overflowing and denormal IQ through the batch, lane by lane against the CPU oracle.

Every GPU test elsewhere feeds well-formed floats.  Here a batch reads the 46 captures of tests/poison.py -- single
infinities and NaNs at every alignment to the resampler's batches of rows, on top of the carried IF history and at the
very end of a call, an overflowing burst, streams in the denormal range, the degenerate kinds and clean stations --
through a capture map that puts clean and poisoned lanes of many kinds into every wave, and every channel of every
call is compared with the oracle decoder of its capture by poison.same_class: equal bits, or NaN for NaN.  There is
no tolerance and no element is left out.  The streams are 0.1 s long: no RDS group completes in them, so the group and
frame comparisons show that a poisoned lane invents none.

Reference: cFmDecoder::ProcessStream and ::Reset (FmDecode.cpp), cDownsampleFilter::Process (DownConvert.cpp:195-233),
CRDSDownConvert::ProcessData (DownConvert.cpp:429-466), RDSProcess.cpp:137-270 as oracle/fmd_oracle.c cites them."""
from importlib import import_module

import numpy as np
import pytest

import poison as P
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
N = P.N


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ref(oracle, fmsig):
    r = P.reference(oracle, fmsig)
    P.assert_not_vacuous(r)
    return r


def _params(pkg, fs=P.FS, d=P.D, order=0):
    return pkg.make_params(fs, P.OFFSET / P.FS * fs, P.PCM, P.BW, d, if_filter_order=order)


def _same(got, want, what):
    assert P.same_class(got, want), (what, P.explain(got, want))


def _same_rows(got, want_rows, what):
    """[C, n] of the batch against the oracle's row of every channel; the message names the first channel that differs"""
    want = np.stack(want_rows)
    if not P.same_class(got, want):
        for c in range(want.shape[0]):
            _same(got[c], want[c], what + (c,))
        _same(got, want, what)


def _strict_rows(got, want_rows, channels, what):
    """clean channels: bit equality outright"""
    for c in channels:
        g, w = np.ascontiguousarray(got[c]), np.ascontiguousarray(want_rows[c])
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), what + (c,)


def _same_status(b, cmap, rec, k, what, channels=None):
    for c in (range(len(cmap)) if channels is None else channels):
        sg, so = b.status(c), rec[cmap[c]][k]["status"]
        assert P.same_status(sg, so), what + (c, list(P.status_floats(sg)), list(P.status_floats(so)))
        assert sg.rds_state == so.rds_state, what + (c, "rds_state")


def _upload(rows, n):
    """[R, 2 n] float32 rows on the device at a stride of a whole number of sample pairs: (tensor, stride in samples)"""
    import torch
    rows = np.ascontiguousarray(rows)
    if n % 2:
        rows = np.concatenate([rows, np.zeros((rows.shape[0], 2), rows.dtype)], axis=1)
    return torch.from_numpy(rows).cuda(), rows.shape[1] // 2


def _layout_batch(pkg, C, k, setup=None, conc=None, taps=False, callbacks=False):
    b = pkg.Batch(_params(pkg), C, record_callbacks=callbacks)
    for key, value in (setup or ()):
        b.debug_set(key, value)
    if taps:
        b.enable_taps()
    if conc is not None:
        b.set_concurrency(conc)
    cmap = P.capture_map(C, k)
    b.set_capture_map(cmap, P.G)
    return b, [int(g) for g in cmap]


def _clean_channels(cmap):
    return [c for c, g in enumerate(cmap) if P.LAYOUT[g].kind not in P.POISONED]


def _tap_channels(cmap):
    """per wave: the first channel on a capture of each group of the layout (a poison inside a call, on the carried
    history, at the end of a call, the burst, the scaled and fading streams, a degenerate kind, a clean station)"""
    groups = [range(0, 16), range(16, 24), range(24, 32), [32], [33], [34], [35], range(36, 42), range(42, 46)]
    pick = []
    for w0 in range(0, len(cmap), 64):
        for gr in groups:
            pick += [c for c in range(w0, min(w0 + 64, len(cmap))) if cmap[c] in gr][:1]
    return pick


def _serial_run(pkg, b, cmap, rows, rec, entry, stages, what):
    """the four calls of the layout one at a time through the host or the device entry point: audio, the five getters
    and the RDS state of every channel, the listed stage taps of _tap_channels, groups (device) or frames (host)"""
    import torch
    C = len(cmap)
    clean, taps_of = _clean_channels(cmap), _tap_channels(cmap)
    st = torch.cuda.current_stream().cuda_stream
    stride = (b.max_audio_floats(N) + 63) // 64 * 64
    groups = []
    for k, n in enumerate(P.SIZES):
        x = np.ascontiguousarray(P.call_rows(rows, k))
        if entry == "host":
            audio = b.process_host(x.view(np.complex64))
        else:
            d_x, xs = _upload(x, n)
            out = torch.zeros((C, stride), dtype=torch.float32, device="cuda")
            nf = b.process_device(d_x.data_ptr(), xs, n, out.data_ptr(), stride, st)
            b.wait(stream=st)
            torch.cuda.synchronize()
            audio = out[:, :nf].cpu().numpy()
            groups += b.collect_rds(stream=st)
        want = [rec[g][k]["audio"] for g in cmap]
        _same_rows(audio, want, what + ("audio", k))
        _strict_rows(audio, want, clean, what + ("clean audio", k))
        _same_status(b, cmap, rec, k, what + ("status", k))
        for c in taps_of:
            for name in stages:
                _same(b.tap(name, c), rec[cmap[c]][k]["taps"][name], what + (name, k, c, cmap[c]))
    if entry == "host":
        for c in range(C):
            assert b.sink.frames.get(c, []) == [f for r in rec[cmap[c]] for f in r["frames"]], what + ("frames", c)
    else:
        for c in range(C):
            got = [blk for ch, _, blk in groups if ch == c]
            assert got == [blk for r in rec[cmap[c]] for blk in r["groups"]], what + ("groups", c)


@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("k", P.K_VALUES)
def test_whole_path_shared_form(pkg, fmsig, ref, k, entry):
    """130 channels (three waves, the last of two lanes), the serial stage in its shared form, taps enabled: every
    stage tap of a channel of each group of the layout per wave, audio, the getters and the RDS state of every
    channel in every call."""
    b, cmap = _layout_batch(pkg, 130, k, taps=True, callbacks=entry == "host")
    _serial_run(pkg, b, cmap, P.captures(fmsig), ref, entry, P.STAGES, (k, entry))
    b.close()


@pytest.mark.parametrize("k", P.K_VALUES)
def test_whole_cu_serial_stage(pkg, fmsig, ref, k):
    """1026 channels at concurrency 2 with three calls in flight: the serial stage in its whole-CU form (two groups per
    workgroup, hand-counted waits, a last workgroup with an empty second group and padded lanes that shadow the last
    channel -- clean for k = 0, poisoned for k = 13).  Audio of every channel and call, getters and groups."""
    import torch
    C = 1026
    b, cmap = _layout_batch(pkg, C, k, conc=2)
    rows = P.captures(fmsig)
    st = torch.cuda.current_stream().cuda_stream
    stride = (b.max_audio_floats(N) + 63) // 64 * 64
    keep, nfs = [], []
    for call, n in enumerate(P.SIZES):
        d_x, xs = _upload(P.call_rows(rows, call), n)
        out = torch.zeros((C, stride), dtype=torch.float32, device="cuda")
        nfs.append(b.process_device(d_x.data_ptr(), xs, n, out.data_ptr(), stride, st))
        keep.append((d_x, out))
        if call >= 2:
            b.wait(stream=st, lag=2)
    b.wait(stream=st)
    torch.cuda.synchronize()
    groups = b.collect_rds(stream=st)
    clean = _clean_channels(cmap)
    for call in range(len(P.SIZES)):
        audio = keep[call][1][:, :nfs[call]].cpu().numpy()
        want = [ref[g][call]["audio"] for g in cmap]
        _same_rows(audio, want, (k, "audio", call))
        _strict_rows(audio, want, clean, (k, "clean audio", call))
    _same_status(b, cmap, ref, len(P.SIZES) - 1, (k, "status"))
    per_channel = {}
    for ch, _, blk in groups:
        per_channel.setdefault(ch, []).append(blk)
    for c in range(C):
        assert per_channel.get(c, []) == [blk for r in ref[cmap[c]] for blk in r["groups"]], (k, "groups", c)
    b.close()


FORMS = {"window": (("resampler", 0),), "ring 8 x 2": (("rsr_form", 0), ("resampler", 1)),
         "ring 4 x 4": (("rsr_form", 1), ("resampler", 1))}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("k", P.K_VALUES)
def test_resampler_forms_against_the_oracle(pkg, fmsig, ref, k, form):
    """The window form and both ring forms of the fractional resampler, each against the oracle (never against each
    other): 130 channels, the onset one baseband row later per capture, i.e. at every alignment to the batches of 8
    rows, the groups of outputs and the ring's segments; the last channel poisoned (k = 0) and clean (k = 13)."""
    b, cmap = _layout_batch(pkg, 130, k, setup=FORMS[form], taps=True, callbacks=True)
    _serial_run(pkg, b, cmap, P.captures(fmsig), ref, "host", ("baseband", "mono_rs", "stereo_rs"), (k, form))
    b.close()


def _point_run(pkg, oracle, fmsig, fs, d, order, C, sizes, points, setup=(), conc=None, ciq=True, stages=()):
    """C channels over the captures of poison.point_case (channel c reads capture c mod their number, each with rows
    of its own: no capture map), device calls, waited for one at a time or -- at concurrency 2 -- at the end.  The
    channel IQ rows of every channel and call against the oracle's demod tap, the audio, and behind the last call the
    getters (interface_level among them)."""
    import torch
    rows, rec = P.point_case(oracle, fmsig, fs, d, sizes, points, order)
    K = rows.shape[0]
    cmap = [c % K for c in range(C)]
    b = pkg.Batch(_params(pkg, fs, d, order), C, record_callbacks=False)
    if conc is not None:
        b.set_concurrency(conc)
    for key, value in setup:
        b.debug_set(key, value)
    if stages:
        b.enable_taps()
    st = torch.cuda.current_stream().cuda_stream
    idx = torch.arange(C, device="cuda") % K
    stride = (b.max_audio_floats(N) + 63) // 64 * 64
    qstride = (b.max_mpx_samples(N) + 3) // 4 * 4 + 12
    keep, counts, start = [], [], 0
    for k, n in enumerate(sizes):
        d_x, xs = _upload(rows[:, 2 * start:2 * (start + n)], n)
        start += n
        d_x = d_x[idx].contiguous()
        out = torch.zeros((C, stride), dtype=torch.float32, device="cuda")
        q = torch.zeros((C, 2 * qstride), dtype=torch.float32, device="cuda") if ciq else None
        r = b.process_device(d_x.data_ptr(), xs, n, out.data_ptr(), stride, st,
                             d_ciq_ptr=q.data_ptr() if ciq else None, ciq_stride=qstride if ciq else 0,
                             ciq=np.complex64 if ciq else None)
        counts.append(r if ciq else (r, 0))
        keep.append((d_x, out, q))
        if conc is None:
            b.wait(stream=st)
            torch.cuda.synchronize()
            _same_status(b, cmap, rec, k, (fs, d, order, "status", k))
            for c in range(min(C, K)):
                for name in stages:
                    _same(b.tap(name, c), rec[c][k]["taps"][name], (fs, d, order, name, k, c))
    b.wait(stream=st)
    torch.cuda.synchronize()
    for k in range(len(sizes)):
        nf, nq = counts[k]
        if ciq:
            got = keep[k][2][:, :2 * nq].cpu().numpy()
            _same_rows(got, [rec[g][k]["taps"]["demod"].view(np.float32) for g in cmap], (fs, d, order, "ciq", k))
        _same_rows(keep[k][1][:, :nf].cpu().numpy(), [rec[g][k]["audio"] for g in cmap], (fs, d, order, "audio", k))
    _same_status(b, cmap, rec, len(sizes) - 1, (fs, d, order, "status"))
    # not vacuous: every poisoned capture's demod tap holds a non-finite value in the call of its point
    for i, (k, s) in enumerate(points):
        assert not np.isfinite(rec[i][k]["taps"]["demod"].view(np.float32)).all() or s >= sizes[k] - d, (i, k, s)
    assert all(np.isfinite(r["taps"]["demod"].view(np.float32)).all() for r in rec[-1])
    b.close()


def _if_points(oracle, fs, d, order, sizes, older=False):
    """where the IF stage's staging can go wrong: the first sample of a call, the lone last sample of an odd-length
    call, the last sample of an even one, both sides of a tile's first output (sample 64 d k + pos), and for the
    long-filter loops the samples just older than that output's window"""
    pos = P.first_output_sample(oracle, fs, d, order)
    border = 64 * d * 8 + pos
    pts = [(0, 0), (0, sizes[0] - 1), (1, 0), (1, sizes[1] - 1), (0, border - 1), (0, border), (0, border + 1)]
    if older:
        o = P.new_oracle(oracle, fs, d, if_filter_order=order)
        taps = o.if_taps().size
        o.close()
        pts += [(0, border - taps), (0, border - taps - 1), (1, border - taps)]
    assert sizes[0] % 2 == 1 and sizes[1] % 2 == 0
    return pts


IF_SIZES = [N - 1, N, 8192]  # an odd call, an even one, a short one that shows what the second carried
IF_FORMS = {
    "k_if_fir": (P.FS, P.D, 0, 24, (), None, False),
    "k_if_fir_mt nt=3": (P.FS, P.D, 0, 1024, (("fir_ro", 1), ("fir_nt", 3)), 2, False),
    "k_if_fir_mt nt=4": (P.FS, P.D, 0, 1024, (("fir_ro", 1), ("fir_nt", 4)), 2, False),
    "k_if_fir_mt nt=8": (P.FS, P.D, 0, 1024, (("fir_ro", 1), ("fir_nt", 8)), 2, False),
    "k_if_fir_mt3 ro=2": (P.FS, P.D, 0, 1024, (("fir_nt", 2), ("fir_ro", 2)), 2, False),
    "k_if_fir_mt3 ro=3": (P.FS, P.D, 0, 1024, (("fir_nt", 2), ("fir_ro", 3)), 2, False),
    "de-interleaved window": (1.0e6, 4, 0, 24, (), None, False),
    "long filter 10 MS/s": (10e6, 46, 4096, 16, (), None, True),
    "long filter 2.4 MS/s": (P.FS, P.D, 2048, 16, (), None, True),
}


@pytest.mark.parametrize("form", list(IF_FORMS))
def test_if_stage_forms(pkg, oracle, fmsig, form):
    """An infinity at the first, the last and the lone odd last sample of a call and on both sides of a tile's border,
    through every form of the IF kernel: the channel IQ rows of all channels against the oracle's demod tap, the audio
    and the getters.  The call after shows the carry."""
    fs, d, order, C, setup, conc, older = IF_FORMS[form]
    _point_run(pkg, oracle, fmsig, fs, d, order, C, IF_SIZES, _if_points(oracle, fs, d, order, IF_SIZES, older),
               setup=setup, conc=conc)


def test_ring_resampler_250_taps(pkg, oracle, fmsig):
    """The ring form at 1.0 MS/s, D = 4 (250 taps: 4 waves x 2 outputs): 16 captures whose onset moves one baseband
    row each, 34 channels, against the oracle."""
    fs, d = 1.0e6, 4
    sizes = [N, N, 40000]
    points = [(1, 30000 + d * g) for g in range(16)]
    _point_run(pkg, oracle, fmsig, fs, d, 0, 34, sizes, points, setup=(("rsr_form", 0), ("resampler", 1)), ciq=False,
               stages=("baseband", "mono_rs", "stereo_rs"))


def test_single_decoder_with_reset(pkg, oracle, fmsig, ref):
    """fmd_process_stream / cFmDecoder: an Inf, Reset(), three more calls; audio and the five getters against the
    oracle after every call.  The reset leaves the decoder poisoned as the reference's does."""
    rows = P.captures(fmsig)
    stream = np.concatenate([rows[0], rows[42][:2 * N]])
    sizes = list(P.SIZES) + [N]
    want = P.run_oracle(oracle, stream, sizes, resets=(2,), taps=False)
    assert not np.isfinite(want[2]["audio"]).any() and not np.isfinite(want[4]["audio"]).any()
    d = pkg.FmDecoder(P.FS, P.OFFSET, P.PCM, P.BW, P.D)
    pos = 0
    for k, n in enumerate(sizes):
        if k == 2:
            d.Reset()
        a = d.ProcessStream(stream[2 * pos:2 * (pos + n)].view(np.complex64))
        pos += n
        _same(a, want[k]["audio"], ("audio", k))
        assert P.same_status(d._status(), want[k]["status"]), ("status", k)
    d.close()


def test_band_scan_with_a_poisoned_capture(pkg, fmsig):
    """Three captures, nfft 1024, a NaN in capture 1: the call returns, psd[1] is NaN in every bin, and the poisoned
    capture reports what include/fmd.h says -- a NaN floor, NaN for every eligible slot and -Inf for the others, no
    candidate.  Captures 0 and 2 have the bits of a scan of the same data without the poison."""
    scanmod = import_module(pkg.__name__ + ".scan")
    rows = P.captures(fmsig)
    x = np.stack([rows[42][:2 * N], rows[43][:2 * N], rows[44][:2 * N]])
    bad = x.copy()
    bad[1, 2 * 12345 + 1] = np.nan
    res = []
    for data in (x, bad):
        s = scanmod.Scan(P.FS, 3, table_size=24, nfft=1024)
        s.accumulate_host(data.view(np.complex64))
        res.append(s.result())
        s.close()
    clean, got = res
    assert np.isfinite(clean["psd"]).all() and all(len(c) > 0 for c in clean["candidates"])
    for g in (0, 2):
        for key in ("psd", "slot_db", "floor_db"):
            a, w = got[key][g], clean[key][g]
            assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(w).tobytes(), (key, g)
        assert got["candidates"][g] == clean["candidates"][g] and got["counts"][g] == clean["counts"][g], g
    assert np.isnan(got["psd"][1]).all()
    assert np.isnan(got["floor_db"][1])
    eligible = np.isfinite(clean["slot_db"][1])
    assert eligible.any() and not eligible.all()
    assert np.isnan(got["slot_db"][1][eligible]).all()
    assert (got["slot_db"][1][~eligible] == -np.inf).all()
    assert got["counts"][1] == 0 and got["candidates"][1] == []


def test_edits_after_the_poison(pkg, oracle, fmsig):
    """Per-channel resets, retunes, capture switches and moves between two batches, each in front of a ragged and in
    front of a full call after a poison in call 1, then a save / load of both batches and a whole-batch reset
    (poison.edit_case): every channel of both batches in every call against the edit model's oracle lineages -- a
    reset slot shows the oracle's partial recovery, NaN for NaN in every tap, also where an earlier reset had put it on
    a ring origin of its own; a retune and an import of a clean decoder revive; a switch to a clean capture does not.
    The same script without its save / load steps delivers the same bytes, NaN payloads included."""
    import edit_model as em
    script, streams, model, shifts, cmaps = P.edit_case(oracle, fmsig)
    taps_of = P.EDIT_TAPS_OF
    results = []
    for with_save in (True, False):
        sc = script if with_save else [(n, [e for e in edits if "save_load" not in e]) for n, edits in script]
        drv = em.Driver(pkg, streams, shifts, cmaps, mode="device", taps_of=taps_of if with_save else (),
                        tap_names=P.EDIT_TAPS, callbacks=False)
        res = drv.play(sc)
        drv.finish()
        results.append(res)
    res, plain = results
    for k in range(len(script)):
        for b in range(2):
            C = model.C[b]
            r = res[k][b]
            _same_rows(r["audio"], [model.at(k, c, b)["audio"] for c in range(C)], ("audio", k, b))
            assert r["audio"].tobytes() == plain[k][b]["audio"].tobytes(), ("save / load", k, b)
            for c in range(C):
                m = model.at(k, c, b)
                assert P.same_status(r["status"][c][0], m["status"]), ("status", k, b, c)
                assert r["status"][c][1] == k + 1, ("status call index", k, b, c)
                assert [blk for ch, _, blk in r["groups"] if ch == c] == m["groups"], ("groups", k, b, c)
            for c in taps_of:
                for t in P.EDIT_TAPS:
                    _same(r["taps"][c][t], model.at(k, c, b)["taps"][t], (t, k, b, c))
    # not vacuous: the reset slots 0 and 2 hold NaNs and finite values in their low-pass tap behind the reset
    for c in (0, 2):
        lpf = res[2][0]["taps"][c]["rds_lpf"].view(np.float32)
        assert np.isnan(lpf).any() and np.isfinite(lpf).any(), c


def _feed_taps(pkg, dv, rate=P.PCM):
    """the feed contract's taps, from the design function (include/fmd.h, FMD_FEED_*; as tests/test_gpu_feed.py)"""
    f = np.float32(rate)
    fo = np.float32(f / np.float32(dv))
    return pkg.design_lp_kaiser(1.0, 60.0, float(np.float32(0.425) * fo), float(np.float32(0.575) * fo), float(f))


@pytest.mark.parametrize("dv,mpx,feed,selected", [(2, np.float32, np.float32, False), (3, np.int16, np.int16, True)])
def test_every_output_format_on_the_poisoned_batch(pkg, fmsig, ref, dv, mpx, feed, selected):
    """130 channels, every call one call record with all four outputs: S16 PCM against the numpy specification on the
    oracle's floats (NaN gives 0, an infinity saturates), the clip counter (a NaN is not a clipped sample), the
    multiplex as float and as S16, the mono feed at both divisors as float and as S16 against tests/feed_spec.py over
    the oracle's audio, the channel IQ as S16, and the audio meter -- with all rows, and with row selections that mix
    clean and poisoned channels."""
    import feed_spec
    from test_mpx_cabi_cpu import mpx16
    from test_pcm_formats_cabi_cpu import clipped, pcm16
    C = 130
    b, cmap = _layout_batch(pkg, C, 0)
    b.set_feed(dv)
    sel = {"audio": list(range(C)), "mpx": list(range(C)), "feed": list(range(C)), "ciq": list(range(C))}
    if selected:
        sel = {"audio": [129, 3, 64, 0, 77], "mpx": [5, 128, 1, 70], "feed": [2, 129, 66, 65, 9], "ciq": [127, 0, 6, 71]}
        assert all({P.LAYOUT[cmap[c]].kind in P.POISONED for c in s} == {True, False} for s in sel.values())
        b.select_audio(sel["audio"])
        b.select_mpx(sel["mpx"])
        b.select_feed(sel["feed"])
        b.select_ciq(sel["ciq"])
    spec = feed_spec.FeedSpec(_feed_taps(pkg, dv), dv, rows=C)
    rows = P.captures(fmsig)
    clip = np.zeros(C, np.uint64)
    level = [np.float32(0)] * C
    saturated = 0
    for k in range(len(P.SIZES)):
        x = np.ascontiguousarray(P.call_rows(rows, k))
        pcm, m, f, q = b.process_host_fmt(x, pcm=np.int16, mpx=mpx, feed=feed, ciq=np.int16)
        audio = [ref[g][k]["audio"] for g in cmap]
        _same_rows(pcm, [pcm16(audio[c]) for c in sel["audio"]], (dv, "pcm", k))
        for c in sel["audio"]:
            clip[c] += np.uint64(clipped(audio[c]).sum())
        base = [ref[cmap[c]][k]["taps"]["baseband"] for c in sel["mpx"]]
        _same_rows(m, base if mpx == np.float32 else [mpx16(r) for r in base], (dv, "mpx", k))
        with np.errstate(invalid="ignore", over="ignore"):
            y = spec.push(np.stack(audio))
        _same_rows(f, [y[c] if feed == np.float32 else feed_spec.s16(y[c]) for c in sel["feed"]], (dv, "feed", k))
        dem = [ref[cmap[c]][k]["taps"]["demod"] for c in sel["ciq"]]
        _same_rows(q, [np.stack([mpx16(r.real), mpx16(r.imag)], axis=-1) for r in dem], (dv, "ciq", k))
        saturated += sum(int((np.abs(mpx16(r.real).astype(np.int32)) >= 32767).sum()) for r in dem)
        for c in range(C):  # the meter belongs to every channel, selected or not
            mean, rms, level[c] = P.audio_meter(audio[c], level[c])
            _same(np.array(b.audio_level(c), np.float32), np.array([mean, rms, level[c]], np.float32),
                  (dv, "meter", k, c))
        _same_status(b, cmap, ref, k, (dv, "status", k))
    got = b.pcm_clipped()
    assert got.dtype == clip.dtype and np.array_equal(got, clip), (dv, np.flatnonzero(got != clip)[:8])
    if not selected:
        assert saturated > 0  # an infinity reached the S16 channel IQ and saturated there
    b.close()


def test_rds_blocks_on_a_poisoned_batch(pkg, oracle, fmsig):
    """fmd_batch_set_rds_blocks(2) on 130 channels of a station with RDS whose decoders are in group decoding when the
    poison arrives in call 14 of 18: records and the eight counters of every channel, the poisoned ones included,
    against tests/rds_sync_spec.py over the oracle's matched-filter and sync taps -- the slicer's compares on NaN."""
    import rds_blocks_cases as cases
    calls, at = 18, 14
    base = fmsig.generate_f32(cases.station_a(fmsig, 0.004), 0, calls * N)
    s0 = at * N
    poison = [("clean", 0, 0, None), ("inf", s0 + 30000, 0, np.inf), ("nan", s0 + 30011, 1, None),
              ("inf", s0 + 30022, 1, -np.inf), ("nan", s0 + 5, 0, None), ("inf", s0 + N - 3, 0, np.inf),
              ("overflow", s0 + 30000, 0, None), ("clean", 0, 0, None)]
    caps = np.stack([P.inject(base, kind, pos, part, value) for kind, pos, part, value in poison])
    want = {}
    for g in range(len(poison) - 1):
        blocks = [caps[g, 2 * k * N:2 * (k + 1) * N] for k in range(calls)]
        want[g] = cases.oracle_spec(oracle, blocks, cases.SHIFT_A, ("poison", g))[0]
    want[len(poison) - 1] = want[0]
    C = 130
    cmap = np.array([(3 * c + 1) % len(poison) for c in range(C)], np.uint32)
    b = pkg.Batch(pkg.make_params(cases.FS, 0.0, P.PCM, P.BW, cases.D, table_size=cases.TABLE), C,
                  tuning_shifts=np.full(C, cases.SHIFT_A, np.int32), record_callbacks=False)
    b.set_capture_map(cmap, len(poison))
    b.set_rds_blocks(pkg.FMD_RDS_BLOCKS_RECORD)
    got, lost_all = [], 0
    for k in range(calls):
        b.process_host_fmt(np.ascontiguousarray(caps[:, 2 * k * N:2 * (k + 1) * N]))
        if k % 6 == 5:
            r, lost = b.collect_rds_blocks(cap=1 << 16)
            got.append(r)
            lost_all += lost
    recs = np.concatenate(got)
    quality = b.rds_quality()
    assert lost_all == 0
    for c in range(C):
        s = want[int(cmap[c])]
        mine = recs[recs["channel"] == c]
        exp = s.records_array().copy()
        exp["channel"] = c
        assert len(mine) == len(exp), (c, len(mine), len(exp))
        bad = np.flatnonzero(mine != exp)
        assert bad.size == 0, (c, bad.size, mine[bad[:3]], exp[bad[:3]])
        assert tuple(int(x) for x in quality[c]) == s.quality(), (c, quality[c], s.quality())
    # not vacuous: the clean decoder delivers groups before and behind call 14; a poisoned one slices no bit behind it
    clean_calls = [ci for ci, _ in want[0].groups]
    assert min(clean_calls) <= at and max(clean_calls) > at + 1, clean_calls
    for g in range(1, len(poison) - 1):
        assert want[g].groups and max(ci for ci, _ in want[g].groups) <= at + 2, g
        assert want[g].q["bits"] < want[0].q["bits"] - 50, g
    b.close()
