"""Every output of a call at random geometries (tests/fuzz_outputs_cases.py), bit for bit against the CPU oracle.

The geometry tests check float audio, getters and groups; the tests of the newer outputs run at 2.4 MS/s, D 11, 48 kHz.
Here a batch of a drawn geometry (IF rate, downsample, filter order, tuner table, CIC stage, byte input, PCM rate,
bandwidth, de-emphasis, channel count, concurrency mode and lag) delivers, call by call through one call record each,
audio as F32 or S16, MPX, feed and channel IQ rows in either format or not at all, with a selection of every row kind
changed in front of one call and a reset, a capture switch or a save / destroy / load in front of another.  Three
channels are compared with `fuzz_outputs_cases.expectations()` with no tolerance: the rows and their counts, feed
taps, status, groups with call index, the clip counter, the block records field by field and the reception counters.
Every row buffer is pre-filled, wider than its rows and holds C + 1 rows whatever the selection: nothing outside the
delivered samples may change.  The same cases looped back through channel IQ rows into a second batch, six of them
through the host entry point, and the comparison itself against five wrong expectations.

Wall time on an MI355X: docs/MEASUREMENTS.md.
"""
import ctypes as C

import numpy as np
import pytest

import fuzz_outputs_cases as fc
import rds_sync_spec as spec
from __graft_entry__ import load_package
from oracle import oracle_py

pytestmark = pytest.mark.gpu

FILL16 = 0x5A5A
FILL32 = 0x5A5A5A5A
CASES = [fc.resolve(k, oracle_py) for k in fc.cases()]
IDS = [fc.case_id(k) for k in CASES]


class _Rows:
    """pre-filled rows on the device: [C + 1, stride] elements of `per` 16- or 32-bit words each, of which the call
    delivers the first n_rows"""

    def __init__(self, all_rows, n_rows, width, s16, per=1):
        import torch
        self.s16, self.per, self.n_rows = bool(s16), per, n_rows
        self.stride = (width + 7) // 8 * 8 + 8
        self.t = torch.full((all_rows + 1, self.stride * per), FILL16 if s16 else FILL32,
                            dtype=torch.int16 if s16 else torch.int32, device="cuda")
        self.count = C.c_uint()

    def clean(self):
        """nothing at or behind the count of a delivered row, and no row behind the delivered ones, has changed"""
        fill, n = (FILL16 if self.s16 else FILL32), self.count.value * self.per
        return bool((self.t[:self.n_rows, n:] == fill).all()) and bool((self.t[self.n_rows:] == fill).all())

    def row(self, i):
        return self.t[i, :self.count.value * self.per].cpu().numpy()


def run_case(pkg, k, blks, ciq_source=None):
    """The resolved case's six calls on a batch (a new batch behind a save); per call {"audio", "mpx", "feed", "ciq":
    rows}, and the final taps, status, groups, clip counts, records and counters.  ciq_source: the per-call rows of
    another run's FMD_CIQ_F32 output, taken as FMD_IN_CIQ_F32 input in place of the IQ."""
    import torch
    Cn, D, fs_if = k["C"], k["D"], k["fs"]
    params = pkg.make_params(fs_if, k["tune"] * fs_if, k["pcm"], k["bw"], D, k["us"], table_size=k["table"],
                             if_filter_order=k["order"])
    sels = fc.selections(k)

    def create(j):
        """a batch set up as the case's is in front of call j"""
        b = pkg.Batch(params, Cn, tuning_shifts=np.full(Cn, k["shift"], np.int32) if k["shared"] else None,
                      record_callbacks=False)
        b.set_concurrency(k["mode"])
        if k["shared"]:
            b.set_capture_map([fc.capture_of(k, c, j) for c in range(Cn)], 3)
        b.set_feed(k["feed_div"])
        b.set_rds_blocks(k["rds_mode"], 1 << 16)
        if j > k["sel_call"]:
            select(b, j)
        return b

    def select(b, j):
        for kind, fn in (("audio", b.select_audio), ("mpx", b.select_mpx), ("feed", b.select_feed),
                         ("ciq", b.select_ciq)):
            if sels[j][kind] is not None:
                fn(sels[j][kind])

    b = create(0)
    smallest, limits = b.min_samples(), b.baseband_limits()
    st = torch.cuda.current_stream().cuda_stream
    fmts = {"audio": {"f32": np.float32, "s16": np.int16}, "mpx": {"f32": np.float32, "s16": np.int16},
            "feed": {"f32": np.float32, "s16": np.int16}, "ciq": {"f32": np.complex64, "s16": np.int16}}
    code = {"audio": pkg.pcm_format_of, "mpx": pkg.mpx_format_of, "feed": pkg.feed_format_of, "ciq": pkg.ciq_format_of}
    station = torch.arange(Cn, device="cuda") % 3
    lag, calls, keep, groups, records, lost, done, saved = k["lag"], [], [], [], [], 0, 0, None

    def collect(lg):
        nonlocal lost
        groups.append(b.collect_rds_array(cap=4 * Cn + 64, stream=st, lag=lg))
        if k["rds_mode"] == 2:
            r, n = b.collect_rds_blocks(cap=1 << 16, lag=lg, stream=st)
            records.append(r)
            lost += n

    def consume(upto, lg):
        nonlocal done
        b.wait(stream=st, lag=lg)
        collect(lg)
        torch.cuda.synchronize()
        for j in range(done, upto):
            for rows in calls[j].values():
                rows.ok = rows.clean()
        done = max(done, upto)

    for j, n in enumerate(k["calls"]):
        if j == k["edit_call"] and k["edit"] == "reset":
            b.reset_channels([k["edit_channel"]])
        elif j == k["edit_call"] and k["edit"] == "switch":
            b.switch_captures([k["edit_channel"]], [fc.capture_of(k, k["edit_channel"], j)])
        elif j == k["edit_call"] and k["edit"] == "save_load":  # save -> destroy -> load into a new batch
            consume(j, 0)
            saved = b.rds_quality()
            blob = b.save_state()
            b.close()
            b = create(j)
            b.load_state(blob)
        if j == k["sel_call"]:
            select(b, j)
        if ciq_source is None:
            pitch = (n + 7) // 8 * 8  # IQ samples from one row to the next
            x = torch.from_numpy(blks[j]).cuda().reshape(3, n, 2)
            d_iq = torch.zeros((3 if k["shared"] else Cn, pitch, 2), dtype=x.dtype, device="cuda")
            d_iq[:, :n] = x if k["shared"] else x[station]
            keep.append(d_iq)
            src = dict(iq=d_iq.data_ptr(), iq_format=pkg.FMD_IQ_U8 if k["u8"] else pkg.FMD_IQ_F32, iq_stride=pitch,
                       samples=n)
        else:
            q = ciq_source[j]
            src = dict(iq=q.t.data_ptr(), iq_format=pkg.FMD_IN_CIQ_F32, iq_stride=q.stride, samples=q.count.value)
        w = k["outs"][j]
        width = {"audio": b.max_audio_floats(n), "mpx": b.max_mpx_samples(n), "feed": max(b.max_feed_samples(n), 1),
                 "ciq": b.max_mpx_samples(n)}
        out, rec = {}, {}
        for kind in fc.KINDS:
            if w[kind] is None:
                continue
            sel = sels[j][kind]
            rows = _Rows(Cn, Cn if sel is None else len(sel), width[kind], w[kind] == "s16", 2 if kind == "ciq" else 1)
            rows.sel = sel
            out[kind] = rows
            rec[kind] = pkg.make_rows(rows.t.data_ptr(), code[kind](fmts[kind][w[kind]]), rows.stride, rows.count)
        torch.cuda.synchronize()
        b.process_call(pkg.make_call(stream=st, **src, **rec))
        calls.append(out)
        if j >= lag:
            consume(j - lag + 1, lag)
    consume(len(calls), 0)
    res = dict(calls=calls, min_samples=smallest, limits=limits, taps=b.feed_taps(), clip=b.pcm_clipped(), lost=lost,
               saved=saved,
               groups=np.concatenate(groups), records=np.concatenate(records) if records else None,
               quality=b.rds_quality(), status={c: b.status(c) for c in fc.checked(k)})
    b.close()
    return res


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view(np.uint8)


def compare(res, exp, if_level=True):
    """the names of the outputs that differ from the expectation (empty: everything is the oracle's, bit for bit);
    if_level=False: but for interface_level, which a call fed channel IQ rows leaves alone"""
    bad, k = [], exp["case"]

    def differ(what, cond):
        if cond and what not in bad:
            bad.append(what)

    differ("feed taps", not np.array_equal(_bits(res["taps"]), _bits(exp["taps"])))
    differ("records lost", res["lost"] != 0)
    g = res["groups"]
    for c, ch in exp["ch"].items():
        for j, (out, want) in enumerate(zip(res["calls"], ch["calls"])):
            for kind, rows in out.items():
                differ("guard of " + kind, not rows.ok)
                e = want[kind]
                n = want["n_audio"] if kind == "audio" else len(e)
                if rows.count.value != n:
                    differ(kind + " count", True)
                    continue
                at = [c] if rows.sel is None else [i for i, ch_i in enumerate(rows.sel) if ch_i == c]
                for i in at:
                    differ("%s %s" % (kind, k["outs"][j][kind]), not np.array_equal(_bits(rows.row(i)), _bits(e)))
        differ("clip count", int(res["clip"][c]) != ch["clip"])
        if g is None:  # the host entry point hands the groups to its own group decoder: the frames that one delivers
            differ("UECP frames", res["uecp"].get(c, []) != ch["uecp"])
        else:
            mine = sorted((int(ci), tuple(int(v) for v in bl))
                          for cc, ci, bl in zip(g["channel"], g["call_index"], g["blocks"]) if cc == c)
            differ("groups", mine != sorted((ci, tuple(bl)) for ci, bl in ch["groups"]))
        s, so = res["status"][c], ch["status"]
        differ("status", bool(s.stereo_detected) != so[0] or any(
            np.float32(a).view(np.uint32) != np.float32(d).view(np.uint32) for a, d in zip(
                so[1 if if_level else 2:], (s.interface_level, s.baseband_level, s.pilot_level,
                                            s.tuning_offset)[0 if if_level else 1:])))
        differ("reception counters", tuple(int(res["quality"][f][c]) for f in spec.QUALITY_FIELDS) != ch["quality"])
        if ch["quality_saved"] is not None:  # the counters of the batch that was saved and destroyed
            differ("reception counters at the save",
                   tuple(int(res["saved"][f][c]) for f in spec.QUALITY_FIELDS) != ch["quality_saved"])
        if k["rds_mode"] == 2:
            r = res["records"]
            r = np.sort(r[r["channel"] == c], order=["call_index", "bit_index"])
            w = ch["records"]
            differ("block records", len(r) != len(w) or any(
                not np.array_equal(r[f].astype(np.int64), w[f].astype(np.int64)) for f in spec.BLOCK_DTYPE.names))
    return bad


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_random_geometry_every_output(oracle, fmsig, case):
    pkg = load_package()
    exp = fc.expectations(case, oracle, fmsig)
    k = exp["case"]
    res = run_case(pkg, k, fc.blocks(k, fmsig))
    q = 8 * k["D"] if k["cic"] else 1  # the short call is the smallest the batch takes (the CIC rule kept)
    assert k["calls"][2] == -(-res["min_samples"] // q) * q and res["min_samples"] == fc.min_samples(k, oracle)
    assert compare(res, exp) == []


LOOP = [(k, i) for k, i in zip(CASES, IDS) if k["loopback"]]


@pytest.mark.parametrize("case", [k for k, _ in LOOP], ids=[i for _, i in LOOP])
def test_loopback_through_channel_iq(oracle, fmsig, case):
    """Batch A decodes the case's IQ and delivers FMD_CIQ_F32 rows of every channel; batch B, of the same parameters,
    takes those device rows as FMD_IN_CIQ_F32 calls on the same stream.  Both are the oracle's bits in every output
    the case draws (B but for interface_level), so B's are A's."""
    pkg = load_package()
    k = dict(case, edit="none", shared=False, shift=0, sel=dict(case["sel"], ciq="none"),
             outs=[dict(o, ciq="f32") for o in case["outs"]])
    exp = fc.expectations(k, oracle, fmsig)
    k = exp["case"]
    a = run_case(pkg, k, fc.blocks(k, fmsig))
    lo, hi, mult = a["limits"]
    for call in exp["ch"][0]["calls"]:  # the generator's mark: every call's M is one the batch takes
        assert lo <= call["M"] <= hi and call["M"] % mult == 0, (call["M"], a["limits"])
    assert compare(a, exp) == []
    b = run_case(pkg, k, None, ciq_source=[out["ciq"] for out in a["calls"]])
    assert compare(b, exp, if_level=False) == []


class _HostRows:
    """pre-filled pageable rows on the host: [C + 1] rows of an odd stride that start on an odd element"""

    def __init__(self, all_rows, n_rows, width, s16, per=1):
        self.s16, self.per, self.n_rows = bool(s16), per, n_rows
        self.stride = (width + 3) | 1
        self.raw = np.full((all_rows + 1) * self.stride * per + 1, FILL16 if s16 else FILL32,
                           np.int16 if s16 else np.int32)
        self.t = self.raw[1:].reshape(all_rows + 1, self.stride * per)
        self.count = C.c_uint()

    def clean(self):
        fill, n = (FILL16 if self.s16 else FILL32), self.count.value * self.per
        return bool((self.t[:self.n_rows, n:] == fill).all() and (self.t[self.n_rows:] == fill).all()
                    and self.raw[0] == fill)

    def row(self, i):
        return self.t[i, :self.count.value * self.per].copy()


def run_case_host(pkg, k, blks):
    """The case's calls through fmd_batch_process_host_call, all four outputs of every call into pageable numpy rows;
    the result has run_case's form."""
    Cn, D, fs_if = k["C"], k["D"], k["fs"]
    params = pkg.make_params(fs_if, k["tune"] * fs_if, k["pcm"], k["bw"], D, k["us"], table_size=k["table"],
                             if_filter_order=k["order"])
    b = pkg.Batch(params, Cn, tuning_shifts=np.full(Cn, k["shift"], np.int32) if k["shared"] else None)
    if k["shared"]:
        b.set_capture_map([c % 3 for c in range(Cn)], 3)
    b.set_feed(k["feed_div"])
    b.set_rds_blocks(k["rds_mode"], 1 << 16)
    sels = fc.selections(k)
    fmts = {"audio": {"f32": np.float32, "s16": np.int16}, "mpx": {"f32": np.float32, "s16": np.int16},
            "feed": {"f32": np.float32, "s16": np.int16}, "ciq": {"f32": np.complex64, "s16": np.int16}}
    code = {"audio": pkg.pcm_format_of, "mpx": pkg.mpx_format_of, "feed": pkg.feed_format_of, "ciq": pkg.ciq_format_of}
    station = np.arange(Cn) % 3
    calls, records, lost = [], [], 0
    for j, n in enumerate(k["calls"]):
        if j == k["sel_call"]:
            for kind, fn in (("audio", b.select_audio), ("mpx", b.select_mpx), ("feed", b.select_feed),
                             ("ciq", b.select_ciq)):
                if sels[j][kind] is not None:
                    fn(sels[j][kind])
        pitch = n + n % 2  # (rows start on a pair of IQ samples)
        x = blks[j].reshape(3, n, 2)
        iq = np.zeros((3 if k["shared"] else Cn, pitch, 2), x.dtype)
        iq[:, :n] = x if k["shared"] else x[station]
        width = {"audio": b.max_audio_floats(n), "mpx": b.max_mpx_samples(n), "feed": max(b.max_feed_samples(n), 1),
                 "ciq": b.max_mpx_samples(n)}
        out, rec = {}, {}
        for kind in fc.KINDS:
            sel, w = sels[j][kind], k["outs"][j][kind]
            rows = _HostRows(Cn, Cn if sel is None else len(sel), width[kind], w == "s16", 2 if kind == "ciq" else 1)
            rows.sel = sel
            out[kind] = rows
            rec[kind] = pkg.make_rows(rows.t.ctypes.data, code[kind](fmts[kind][w]), rows.stride, rows.count)
        call = pkg.make_call(iq.ctypes.data, pkg.FMD_IQ_U8 if k["u8"] else pkg.FMD_IQ_F32, pitch, n, **rec)
        pkg._check(pkg.lib().fmd_batch_process_host_call(b._h, C.byref(call)))
        for rows in out.values():
            rows.ok = rows.clean()
        calls.append(out)
        if k["rds_mode"] == 2:
            r, nl = b.collect_rds_blocks(cap=1 << 16)
            records.append(r)
            lost += nl
    res = dict(calls=calls, taps=b.feed_taps(), clip=b.pcm_clipped(), lost=lost, saved=None,
               groups=None, uecp=dict(b.sink.frames), records=np.concatenate(records) if records else None,
               quality=b.rds_quality(), status={c: b.status(c) for c in fc.checked(k)})
    b.close()
    return res


HOST = [i for i in (2, 9, 13, 16, 26, 30) if i < len(CASES)]  # the PCM rates, a CIC stage, 4096 taps, 1 to 130 channels


@pytest.mark.parametrize("case", [CASES[i] for i in HOST], ids=[IDS[i] for i in HOST])
def test_host_entry_points_same_bits(oracle, fmsig, case):
    """Six of the cases through the host entry point, every call with all four outputs (a kind the case leaves out
    of a call: as float) from pageable numpy rows of odd stride on an odd element: the bits the device calls of
    test_random_geometry_every_output are held to -- the oracle's --, so the staging copies, whose sizes follow the
    geometry's largest M and frame count, deliver what the device rows hold."""
    pkg = load_package()
    k = dict(case, edit="none", outs=[{kind: o[kind] or "f32" for kind in fc.KINDS} for o in case["outs"]])
    exp = fc.expectations(k, oracle, fmsig)
    assert compare(run_case_host(pkg, exp["case"], fc.blocks(exp["case"], fmsig)), exp) == []


def test_the_comparison_reports_a_wrong_expectation(oracle, fmsig):
    """Teeth: one cheap case run once, then held against expectations that are wrong in the smallest way; each must be
    reported, under the right output's name."""
    pkg = load_package()
    k = dict(fc.case(1), C=3, calls=[20000, 13001, 8192, 9999, 20000, 7777], pcm=44100.0, order=0, rds_mode=1,
             edit="none", cic=False, shared=False, shift=0, loud=True)
    k["outs"] = [dict(audio=("f32", "s16")[j % 2], mpx=("f32", "s16")[j % 2], feed=("s16", "f32")[j % 2], ciq="f32")
                 for j in range(6)]
    assert k["calls"][0] <= 32700 * k["D"]
    exp = fc.expectations(k, oracle, fmsig)
    res = run_case(pkg, k, fc.blocks(k, fmsig))
    assert compare(res, exp) == []
    assert exp["ch"][0]["clip"] > 0
    # a FeedSpec whose frame count starts one frame late
    late = compare(res, fc.expectations(k, oracle, fmsig, feed_late=1))
    assert late and set(late) <= {"feed count", "feed f32", "feed s16"}
    # MPX expected one sample early
    early = fc.expectations(k, oracle, fmsig)
    for ch in early["ch"].values():
        for call in ch["calls"]:
            call["mpx"] = np.concatenate([call["mpx"][1:], call["mpx"][-1:]])
    assert set(compare(res, early)) == {"mpx f32", "mpx s16"}
    # an S16 rule that rounds half away from zero
    away, ties = fc.expectations(k, oracle, fmsig), 0
    for c, ch in away["ch"].items():
        for j, call in enumerate(ch["calls"]):
            if k["outs"][j]["mpx"] == "s16":
                y = call["mpx_f32"].astype(np.float64) * 8192.0
                ties += int((np.abs(y) % 1.0 == 0.5).sum())
                call["mpx"] = np.clip(np.sign(y) * np.floor(np.abs(y) + 0.5), -32768, 32767).astype(np.int16)
    print("S16 MPX samples on a tie:", ties)
    assert ties > 0 and compare(res, away) == ["mpx s16"]
    # a 48 kHz oracle against a 44.1 kHz batch
    other = compare(res, fc.expectations(k, oracle, fmsig, pcm=48000.0))
    assert "audio count" in other and not any(n.startswith(("mpx", "ciq", "feed taps")) for n in other)
    # a clip count that includes the float calls
    assert compare(res, fc.expectations(k, oracle, fmsig, clip_all=True)) == ["clip count"]
