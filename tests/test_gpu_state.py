"""Saving and restoring a running batch, moving live channels between batches (fmd_batch_save_state / _load_state /
_export_channels / _import_channels, include/fmd.h), bit for bit.

A restored or moved decoder must produce the bits of the decoder that was never interrupted: every comparison here
is an equality against a run of the same batch without the interruption (and, as an anchor, against the oracle
decoder).  The stations and helpers are those of tests/test_gpu_reset_channels.py: 8 channels with SHIFTS0 on one
shared capture, calls of 65 536 samples, a tuner table of 24 entries."""
import numpy as np
import pytest
import torch

from __graft_entry__ import load_package
from test_gpu_reset_channels import (FS, D, N, SHIFTS0, T, _bits, _capture, _oracle, _oracle_run, _params,
                                     _stations)

pytestmark = pytest.mark.gpu

NBLK, K = 28, 12  # calls of the long runs; the save / the move is in front of call K
MOVE_END = 24     # calls of the runs with two batches
C8 = len(SHIFTS0)
# batch B of the moves: other shifts (slots 6, 2 and 3 on empty steps of its own capture), its own capture in row 1
SHIFTS_B = [2, -4, 9, -9, 5, -2, 11, 6]
FMD_ERR_ARG, FMD_ERR_STATE = "fmd error -1", "fmd error -4"


class _Log(dict):
    """the callback sink's name table, keeping every name that arrived"""

    def __init__(self):
        super().__init__()
        self.log = {}

    def __setitem__(self, ch, name):
        self.log.setdefault(ch, []).append(name)
        super().__setitem__(ch, name)


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def caps(fmsig):
    """the shared capture of batch A, block by block (float32 I, Q pairs)"""
    st = _stations(fmsig)
    return [_capture(st, fmsig, j) for j in range(NBLK)]


@pytest.fixture(scope="module")
def caps_b(fmsig):
    """batch B's own capture: one stereo + RDS station at -500 kHz (channel 4 of SHIFTS_B tunes it)"""
    p = fmsig.default_params(FS, f_offset=-500e3, amp=0.25, noise_sigma=0.004, seed=97, pi=0x7044, ps="BSIDE")
    return [fmsig.generate_f32(p, j * N, N) for j in range(MOVE_END)]


def _u8(cap):
    """the capture as RTL-SDR byte pairs"""
    return np.clip(np.round(cap * 127.5 + 127.5), 0, 255).astype(np.uint8)


class Run:
    """A batch driven through device calls, every call's observable outputs recorded: audio of every channel, the
    getters, the status call index, the audio meter, the RDS groups with their call index, UECP frames and names."""

    def __init__(self, pkg, shifts=SHIFTS0, enable=False, debug=None, conc=None, prof=None, pcm=None, cmap=None,
                 n_cap=1, params=None, taps=False, keep_phase=False, callbacks=True):
        self.pkg, self.pcm, self.C = pkg, pcm, len(shifts)
        self.b = pkg.Batch(params or _params(pkg), self.C, tuning_shifts=np.array(shifts, np.int32),
                           record_callbacks=callbacks)
        if callbacks:
            self.b.sink.names = _Log()
        if enable:
            self.b.enable_retune()
        for k, v in (debug or {}).items():
            self.b.debug_set(k, v)
        if keep_phase:
            self.b.debug_reset_keep_ring_phase(1)
        if taps:
            self.b.enable_taps(True)
        if conc is not None:
            self.b.set_concurrency(conc)
        if prof is not None:
            self.b.set_profiling(prof)
        self.n_cap = n_cap
        if cmap is not None:
            self.b.set_capture_map(cmap, n_cap)
        self.stride = (self.b.max_audio_floats(N) + 63) // 64 * 64
        self.s = torch.cuda.current_stream().cuda_stream
        self.rec = []

    def submit(self, block, samples=None):
        """one call without waiting; block: [n_cap, 2 n] float32 / uint8 rows (one row: shared); with `samples`, the
        rows are longer than the call (a row stride of its own).  Returns what finish() needs."""
        x = torch.from_numpy(np.ascontiguousarray(block)).cuda()
        rows = x.reshape(self.n_cap, -1)
        stride = rows.shape[1] // 2
        n = stride if samples is None else samples
        out = torch.zeros((self.C, self.stride), dtype=torch.int16 if self.pcm else torch.float32, device="cuda")
        fmt = self.pkg.FMD_IQ_U8 if x.dtype == torch.uint8 else self.pkg.FMD_IQ_F32
        nf = self.b.process_device(rows.data_ptr(), stride if self.n_cap > 1 else 0, n, out.data_ptr(), self.stride,
                                   self.s, fmt=fmt, pcm=np.int16 if self.pcm else None)
        return x, out, nf

    def getters(self):
        g = []
        for c in range(self.C):
            s = self.b.status(c)
            f = np.array([s.tuning_offset, s.interface_level, s.baseband_level, s.pilot_level,
                          *self.b.audio_level(c)], np.float32)
            g.append((int(s.stereo_detected), int(s.rds_state), self.b.status_call_index(c), f.tobytes()))
        return g

    def finish(self, pending):
        _, out, nf = pending
        self.b.wait(stream=self.s)
        torch.cuda.synchronize()
        groups = self.b.collect_rds(run_group_decoder=True, stream=self.s)
        r = {"audio": out[:, :nf].cpu().numpy(), "groups": groups, "getters": self.getters(),
             "nframes": [len(self.b.sink.frames.get(c, [])) for c in range(self.C)],
             "nnames": [len(self.b.sink.names.log.get(c, [])) for c in range(self.C)]}
        self.rec.append(r)
        return r

    def call(self, block):
        return self.finish(self.submit(block))

    def frames(self, c, since=0):
        return self.b.sink.frames.get(c, [])[since:]

    def names(self, c, since=0):
        return self.b.sink.names.log.get(c, [])[since:]

    def close(self):
        self.b.close()


def _same_audio(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _groups_of(groups, c, as_c=None):
    return [(c if as_c is None else as_c, k, blk) for ch, k, blk in groups if ch == c]


def _assert_same_call(got, want, j, pairs=None):
    """every recorded output of call j: channel g of `got` against channel w of `want` for (g, w) in pairs"""
    pairs = pairs if pairs is not None else [(c, c) for c in range(got["audio"].shape[0])]
    for g, w in pairs:
        assert _same_audio(got["audio"][g], want["audio"][w]), ("audio", j, g, w)
        assert got["getters"][g] == want["getters"][w], ("getters", j, g, w)
        assert _groups_of(got["groups"], g, w) == _groups_of(want["groups"], w), ("groups", j, g, w)


@pytest.fixture(scope="module")
def ref(pkg, caps):
    """batch A never interrupted, all NBLK calls: what every continuation below is compared with"""
    r = Run(pkg)
    for j in range(NBLK):
        r.call(caps[j])
    out = {"rec": r.rec, "frames": {c: r.frames(c) for c in range(C8)}, "names": {c: r.names(c) for c in range(C8)}}
    r.close()
    return out


@pytest.fixture(scope="module")
def anchor(oracle, caps):
    """the oracle decoder of channel 0 on the same capture"""
    o, out, taps = _oracle_run(oracle, SHIFTS0[0], caps)
    return {"audio": out, "frames": o.uecp_frames(), "name": o.channel_name(),
            "rds_rows": [len(t["rds_mf"]) for t in taps]}


@pytest.fixture(scope="module")
def saved(pkg, caps, ref):
    """batch A saved behind call K - 1 (groups collected first), then destroyed"""
    src = Run(pkg)
    for j in range(K):
        _assert_same_call(src.call(caps[j]), ref["rec"][j], j)
    blob = src.b.save_state()
    getters = src.getters()
    src.close()
    return {"blob": blob, "getters": getters}


def _assert_continues(dst, ref, caps, first, last, frames_since=None):
    """dst's calls first..last - 1 and everything its callbacks received equal the uninterrupted run's"""
    for j in range(first, last):
        _assert_same_call(dst.call(caps[j]), ref["rec"][j], j)
    at, end = ref["rec"][first - 1], ref["rec"][last - 1]
    for c in range(C8):
        assert dst.frames(c) == ref["frames"][c][at["nframes"][c]:end["nframes"][c]], ("frames", c)
        assert dst.names(c) == ref["names"][c][at["nnames"][c]:end["nnames"][c]], ("names", c)


def test_continuation_after_destroy_is_exact(pkg, oracle, caps, ref, anchor, saved):
    """28 calls with a save behind call 11: the RDS ring phases there are non-zero (asserted), the batch is destroyed,
    a fresh one loads the blob and runs calls 12-27.  Every channel equals the uninterrupted batch in the audio of
    every call, the getters right after the load (the source's at the save) and after every call, the status call
    index, the collected RDS groups with their call index, UECP frames (one begun before the save completes after
    the load), PS names and the audio meter.  Channel 0 also equals the oracle decoder."""
    n = sum(anchor["rds_rows"][:K])
    o = _oracle(oracle, 0)
    assert n % len(o.rds_lpf_taps()) != 0 and n % len(o.rds_mf_taps()) != 0
    assert saved["getters"] == ref["rec"][K - 1]["getters"]
    dst = Run(pkg)
    dst.b.load_state(saved["blob"])
    assert dst.getters() == saved["getters"]
    _assert_continues(dst, ref, caps, K, NBLK)
    for j in range(K, NBLK):
        assert _bits(dst.rec[j - K]["audio"][0], anchor["audio"][j]), j
    assert ref["frames"][0][:ref["rec"][K - 1]["nframes"][0]] + dst.frames(0) == anchor["frames"]
    assert len(dst.frames(0)) > 0
    if anchor["name"].strip():
        assert (ref["names"][0][:ref["rec"][K - 1]["nnames"][0]] + dst.names(0))[-1] == anchor["name"]
    dst.close()


DST_FORMS = {"concurrency0": dict(conc=0), "profiling2": dict(prof=2), "ring4_off": dict(debug={"ring4": 0}),
             "resampler_ring": dict(debug={"resampler": 1}), "resampler_window": dict(debug={"resampler": 0}),
             "halfband_chain": dict(debug={"halfband_chain": 1}), "halfband_stages": dict(debug={"halfband_chain": 0})}


@pytest.mark.parametrize("form", sorted(DST_FORMS))
def test_destination_form_does_not_matter(pkg, caps, ref, saved, form):
    """The state is independent of the kernel form and the stream layout: the destination runs at concurrency 0, at
    profiling level 2, with the LDS form of the ring filters, with either resampler and either half-band form (the
    one-launch chain keeps the batch-wide oscillator sequence, which the source did not) -- six calls, exact."""
    dst = Run(pkg, **DST_FORMS[form])
    dst.b.load_state(saved["blob"])
    assert dst.getters() == saved["getters"]
    _assert_continues(dst, ref, caps, K, K + 6)
    dst.close()


@pytest.mark.parametrize("form", ["u8", "s16", "source_in_flight", "source_chain"])
def test_source_forms(pkg, fmsig, caps, ref, form):
    """Byte input; FMD_PCM_S16 output of an over-deviated station whose audio saturates all along, so that the clipped
    counts are non-zero at the save, grow behind the load and end at the uninterrupted run's; a source at concurrency 2 with three calls
    in flight when save_state is called (it waits for them); a source that keeps the oscillator sequence loaded into
    one that does not.  16 calls, the save behind call 11."""
    kw = dict(pcm=True) if form == "s16" else {}
    skw = dict(debug={"halfband_chain": 1}) if form == "source_chain" else {}
    blocks = [_u8(c) for c in caps[:16]] if form == "u8" else caps[:16]
    if form == "s16":
        hot = fmsig.default_params(FS, f_offset=-700e3, amp=0.3, noise_sigma=0.004, seed=91, pi=0x7011, ps="LOUD",
                                   dev=150e3)
        blocks = [fmsig.generate_f32(hot, j * N, N) for j in range(16)]
    if form in ("u8", "s16"):
        whole = Run(pkg, **kw)
        for j in range(16):
            whole.call(blocks[j])
        want = {"rec": whole.rec, "frames": {c: whole.frames(c) for c in range(C8)},
                "names": {c: whole.names(c) for c in range(C8)}}
        clipped = whole.b.pcm_clipped()
        whole.close()
    else:
        want = ref
    src = Run(pkg, **kw, **skw)
    if form == "source_in_flight":
        src.b.set_concurrency(2)
        for j in range(K - 3):
            src.call(blocks[j])
        pend = [src.submit(blocks[j]) for j in range(K - 3, K)]
        blob = src.b.save_state()  # waits for the three calls
        for j, p in zip(range(K - 3, K), pend):
            assert _same_audio(p[1][:, :p[2]].cpu().numpy(), want["rec"][j]["audio"]), j
        # (their groups stay in the source: collected here, they are the uninterrupted run's)
        got = src.b.collect_rds(run_group_decoder=False, stream=src.s)
        assert got == [g for j in range(K - 3, K) for g in want["rec"][j]["groups"]]
    else:
        for j in range(K):
            _assert_same_call(src.call(blocks[j]), want["rec"][j], j)
        blob = src.b.save_state()
        clipped_at_save = src.b.pcm_clipped()
    src.close()
    dst = Run(pkg, **kw)
    dst.b.load_state(blob)
    if form == "s16":
        assert np.array_equal(dst.b.pcm_clipped(), clipped_at_save)
    if form == "source_in_flight":
        # the source's group decoders had not seen the three calls' groups: neither has the destination's
        for j in range(K, 16):
            r = dst.call(blocks[j])
            for c in range(C8):
                assert _same_audio(r["audio"][c], want["rec"][j]["audio"][c]), (j, c)
                assert r["getters"][c] == want["rec"][j]["getters"][c], (j, c)
            assert r["groups"] == want["rec"][j]["groups"], j
    else:
        _assert_continues(dst, want, blocks, K, 16)
    if form == "s16":
        print("clipped at the save", clipped_at_save, "at the end", clipped)
        assert clipped_at_save[0] > 0 and clipped[0] > clipped_at_save[0]
        assert np.array_equal(dst.b.pcm_clipped(), clipped)
    dst.close()


def _history_edits(r, j):
    """what the source of the history test has been through, in front of call j"""
    if j == 3:
        r.b.reset_channels([1, 4, 6])
    if j == 5:
        r.b.retune([3, 7], [7, -5])
    if j == 6:
        r.b.switch_captures([2, 5], [1, 0])
    if j == 10:
        r.b.retune([2], [7])


def test_history_resets_retunes_and_switches(pkg, caps, caps_b):
    """Before the save the source has had reset_channels on three channels (the ring origins are live), retunes with
    retuning enabled (the silent twin is part of the blob) and a capture map over two rows with switches.  The
    continuation is exact, a retune behind the load equals the uninterrupted batch's retune, and a destination
    without enable_retune is refused with FMD_ERR_STATE."""
    cmap = [0, 0, 0, 0, 1, 1, 0, 0]
    nblk, k = 13, 8
    blocks = [np.stack([caps[j], caps_b[j]]) for j in range(nblk)]

    def make():
        return Run(pkg, enable=True, cmap=cmap, n_cap=2)

    whole = make()
    for j in range(nblk):
        _history_edits(whole, j)
        whole.call(blocks[j])
    want = {"rec": whole.rec, "frames": {c: whole.frames(c) for c in range(C8)},
            "names": {c: whole.names(c) for c in range(C8)}}
    whole.close()
    src = make()
    for j in range(k):
        _history_edits(src, j)
        src.call(blocks[j])
    blob = src.b.save_state()
    getters = src.getters()
    src.close()
    plain = Run(pkg, cmap=cmap, n_cap=2)
    with pytest.raises(pkg.FmdError, match=FMD_ERR_STATE):
        plain.b.load_state(blob)
    plain.close()
    dst = Run(pkg, enable=True, n_cap=2, cmap=[0] * C8)  # (the map is the blob's)
    dst.b.load_state(blob)
    assert dst.getters() == getters
    assert list(dst.b.capture_map()[0]) == [0, 0, 1, 0, 1, 0, 0, 0]
    for j in range(k, nblk):
        _history_edits(dst, j)
        _assert_same_call(dst.call(blocks[j]), want["rec"][j], j)
    at = want["rec"][k - 1]
    for c in range(C8):
        assert dst.frames(c) == want["frames"][c][at["nframes"][c]:], c
        assert dst.names(c) == want["names"][c][at["nnames"][c]:], c
    dst.close()


def test_sub_batches_and_import_into_the_second(pkg, caps):
    """A shell of 16 384 channels (two sub-batches), calls of 8192 samples: two before the save, two after, compared
    with the uninterrupted shell in one channel per sub-batch and the shell's first and last channel.  Then channels
    0 and 8191 are exported and imported into slots 9000 and 16 001 of the second sub-batch (the same shell: its
    clock is the blob's, and every channel reads the one shared capture): from the next call on the slots are the
    exported channels."""
    C_, n = 16384, 8192
    shifts = np.resize(np.array(SHIFTS0, np.int32), C_)
    look = [0, 5000, 8191, 8192, 12000, 16383]
    dev = [torch.from_numpy(caps[0][2 * n * j:2 * n * (j + 1)].copy()).cuda() for j in range(5)]

    def make():
        return pkg.Batch(_params(pkg), C_, tuning_shifts=shifts, record_callbacks=False)

    def call(b, j):
        stride = (b.max_audio_floats(n) + 63) // 64 * 64
        out = torch.zeros((C_, stride), dtype=torch.float32, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        nf = b.process_device(dev[j].data_ptr(), 0, n, out.data_ptr(), stride, s)
        b.wait(stream=s)
        torch.cuda.synchronize()
        st = [(b.status(c).stereo_detected, np.float32(b.status(c).interface_level).tobytes(),
               b.status_call_index(c)) for c in look]
        return out[:, :nf].cpu().numpy(), st

    whole = make()
    want = [call(whole, j) for j in range(5)]
    whole.close()
    src = make()
    for j in range(2):
        call(src, j)
    blob = src.save_state()
    src.close()
    dst = make()
    dst.load_state(blob)
    del blob
    for j in range(2, 4):
        a, st = call(dst, j)
        assert np.array_equal(a[look].view(np.uint32), want[j][0][look].view(np.uint32)), j
        assert st == want[j][1], j
    moved = dst.export_channels([0, 8191])
    dst.import_channels([16001, 9000], moved)
    a, _ = call(dst, 4)
    keep = np.ones(C_, bool)
    keep[[16001, 9000]] = False
    assert np.array_equal(a[keep].view(np.uint32), want[4][0][keep].view(np.uint32))
    assert _bits(a[16001], want[4][0][0]) and _bits(a[9000], want[4][0][8191])
    assert not _bits(a[16001], want[4][0][16001])
    dst.close()


def _differs(dst, ref, caps, saved, calls=NBLK - K):
    """does any recorded output of the loaded batch differ from the uninterrupted run within `calls` calls?  Says
    where first (None: nowhere)."""
    if dst.getters() != saved["getters"]:
        return "getters right after the load"
    at = ref["rec"][K - 1]
    for j in range(K, K + calls):
        got, want = dst.call(caps[j]), ref["rec"][j]
        for what in ("audio", "getters", "groups"):
            same = _same_audio(got[what], want[what]) if what == "audio" else got[what] == want[what]
            if not same:
                return "%s of call %d" % (what, j)
        for c in range(C8):
            if dst.frames(c) != ref["frames"][c][at["nframes"][c]:want["nframes"][c]] or \
                    dst.names(c) != ref["names"][c][at["nnames"][c]:want["nnames"][c]]:
                return "callbacks of channel %d behind call %d" % (c, j)
    return None


def _used_destination(pkg, caps):
    """a destination that has been decoding something else: two calls on later blocks of the capture.  A load has to
    replace all of it; what a skipped region leaves behind is that other decoder's, not a fresh batch's zeros."""
    dst = Run(pkg)
    for j in (20, 21):
        dst.call(caps[j])
    dst.rec.clear()
    dst.b.sink.frames.clear()
    dst.b.sink.names.log.clear()
    return dst


@pytest.mark.parametrize("region", list(range(11)))
def test_every_region_matters(pkg, caps, ref, saved, region):
    """fmd_batch_debug_state_skip(region) before the load leaves one region of the record out (0-7 the carried device
    regions, 8 the status record, 9 the group decoder, 10 the audio meter and clip counter): some output of some
    channel then differs from the uninterrupted run within the remaining 16 calls (the run stops at the first
    difference).  The destination has decoded two other blocks before.  No region is exempt."""
    dst = _used_destination(pkg, caps)
    dst.b.debug_state_skip(region)
    dst.b.load_state(saved["blob"])
    where = _differs(dst, ref, caps, saved)
    print("region %d: first difference in %s" % (region, where))
    assert where is not None, region
    dst.close()


def test_no_region_skipped_is_exact_again(pkg, caps, ref, saved):
    """... and with -1 the same used destination is exact again: the load replaces everything it held."""
    dst = _used_destination(pkg, caps)
    dst.b.debug_state_skip(3)
    dst.b.debug_state_skip(-1)
    dst.b.load_state(saved["blob"])
    assert _differs(dst, ref, caps, saved, 4) is None
    with pytest.raises(pkg.FmdError, match="region"):
        dst.b.debug_state_skip(11)
    dst.close()


def test_blob_hygiene(pkg, caps, ref, saved):
    """Two saves with no call in between are byte-identical, and so is a save behind a load; one flipped payload
    byte, one flipped header byte and a truncated blob each give FMD_ERR_ARG, as do a blob of another geometry
    (downsample 10) and one of another channel count, and the destination then continues as if nothing had been
    attempted; a save with a pending edit gives FMD_ERR_STATE."""
    live = Run(pkg)
    for j in range(K):
        live.call(caps[j])
    s1 = live.b.save_state()
    assert s1 == live.b.save_state()
    assert s1 == saved["blob"]  # (another batch with the same history: nothing of the process is in the blob)
    assert len(s1) == pkg.lib().fmd_batch_state_size(live.b._h, C8)
    other = Run(pkg)
    other.b.load_state(s1)
    assert other.b.save_state() == s1
    other.close()
    bad = bytearray(s1)
    bad[len(bad) - 1000] ^= 0x10
    flipped_payload = bytes(bad)
    bad = bytearray(s1)
    bad[70] ^= 0x01
    flipped_header = bytes(bad)
    odd = Run(pkg, params=pkg.make_params(FS, 0.0, 48000.0, 15000.0, 10, table_size=T))
    odd.call(caps[0])
    other_geometry = odd.b.save_state()
    odd.close()
    few = Run(pkg, shifts=SHIFTS0[:4])
    few.call(caps[0])
    other_count = few.b.save_state()
    few.close()
    for blob, word in ((flipped_payload, "checksum"), (flipped_header, "checksum"), (s1[:-8], "truncated"),
                       (s1[:200], ""), (other_geometry, "geometry"), (other_count, "channels")):
        with pytest.raises(pkg.FmdError, match=FMD_ERR_ARG) as e:
            live.b.load_state(blob)
        assert word in str(e.value), (word, str(e.value))
    live.b.reset_channels([1])
    with pytest.raises(pkg.FmdError, match=FMD_ERR_STATE):
        live.b.save_state()
    twin = Run(pkg)  # the same batch without the attempts: the reset included
    for j in range(K):
        twin.call(caps[j])
    twin.b.reset_channels([1])
    for j in range(K, K + 3):
        _assert_same_call(live.call(caps[j]), twin.call(caps[j]), j)
    live.close()
    twin.close()


@pytest.fixture(scope="module")
def ref_b(pkg, caps, caps_b):
    """batch B without an import: MOVE_END calls on the two capture rows, every channel on its own capture (row 1)"""
    r = Run(pkg, shifts=SHIFTS_B, cmap=[1] * C8, n_cap=2)
    for j in range(MOVE_END):
        r.call(np.stack([caps[j], caps_b[j]]))
    out = {"rec": r.rec, "frames": {c: r.frames(c) for c in range(C8)}, "names": {c: r.names(c) for c in range(C8)}}
    r.close()
    return out


MOVED = [(6, 0), (2, 1), (3, 5)]  # (slot of B, channel of A)


def _run_a_and_b(pkg, caps, caps_b, upto):
    a = Run(pkg)
    b = Run(pkg, shifts=SHIFTS_B, cmap=[1] * C8, n_cap=2)
    for j in range(upto):
        a.call(caps[j])
        b.call(np.stack([caps[j], caps_b[j]]))
    return a, b


def test_moving_channels_between_batches(pkg, oracle, caps, caps_b, ref, ref_b, anchor):
    """A and B, 8 channels each with different shifts; B reads a map over two rows (A's capture, its own).  Before
    call 12 A's channels 0, 1, 5 are exported, imported into B's slots 6, 2, 3 and those slots switched to A's
    capture.  From call 12 on the slots equal A's channels continuing (audio, getters, groups, frames, names), slot 6
    also the oracle decoder of A's shift on A's capture; B's other channels equal B without the import; A goes on
    unaffected."""
    a, b = _run_a_and_b(pkg, caps, caps_b, K)
    blob = a.b.export_channels([w for _, w in MOVED])
    before = {g: (len(b.frames(g)), len(b.names(g))) for g, _ in MOVED}
    b.b.import_channels([g for g, _ in MOVED], blob)
    b.b.switch_captures([g for g, _ in MOVED], [0, 0, 0])
    others = [(c, c) for c in range(C8) if c not in [g for g, _ in MOVED]]
    for j in range(K, MOVE_END):
        _assert_same_call(a.call(caps[j]), ref["rec"][j], j)
        got = b.call(np.stack([caps[j], caps_b[j]]))
        _assert_same_call(got, ref["rec"][j], j, MOVED)
        _assert_same_call(got, ref_b["rec"][j], j, others)
        assert _bits(got["audio"][6], anchor["audio"][j]), j
    at, end = ref["rec"][K - 1], ref["rec"][MOVE_END - 1]
    for g, w in MOVED:
        assert b.frames(g, before[g][0]) == ref["frames"][w][at["nframes"][w]:end["nframes"][w]], (g, w)
        assert b.names(g, before[g][1]) == ref["names"][w][at["nnames"][w]:end["nnames"][w]], (g, w)
    assert len(b.frames(6, before[6][0])) > 0
    for c, _ in others:
        assert b.frames(c) == ref_b["frames"][c], c
    a.close()
    b.close()


def test_import_order_with_resets(pkg, oracle, caps, caps_b, ref):
    """Edits of one slot before one call apply in the order made: reset_channels then import is the import (slot 2);
    import then reset_channels is the imported decoder reset at call 12 -- the oracle decoder of A's channel 0 with
    reset() there (slot 6)."""
    a, b = _run_a_and_b(pkg, caps, caps_b, K)
    blob = a.b.export_channels([w for _, w in MOVED])
    b.b.reset_channels([2])
    b.b.import_channels([g for g, _ in MOVED], blob)
    b.b.reset_channels([6])
    b.b.switch_captures([g for g, _ in MOVED], [0, 0, 0])
    o, out, _ = _oracle_run(oracle, SHIFTS0[0], caps[:16], resets=(K,))
    n6 = len(b.frames(6))
    for j in range(K, 16):
        got = b.call(np.stack([caps[j], caps_b[j]]))
        _assert_same_call(got, ref["rec"][j], j, [(2, 1), (3, 5)])
        assert _bits(got["audio"][6], out[j]), j
    # the oracle's frames behind its reset: its group decoder starts afresh there like the slot's
    o2 = _oracle(oracle, SHIFTS0[0])
    for j in range(K):
        o2.process_stream(caps[j])
    assert b.frames(6, n6) == o.uecp_frames()[len(o2.uecp_frames()):]
    a.close()
    b.close()


@pytest.mark.parametrize("lag", [1, 2, 3])
def test_import_with_calls_in_flight(pkg, caps, caps_b, ref, ref_b, lag):
    """B at concurrency 2 with `lag` calls in flight when the import is made: the calls in flight keep the old
    occupant, the slots are A's channels from the next call submitted."""
    a = Run(pkg)
    b = Run(pkg, shifts=SHIFTS_B, cmap=[1] * C8, n_cap=2, conc=2)
    for j in range(K):
        a.call(caps[j])
    for j in range(K - lag):
        b.call(np.stack([caps[j], caps_b[j]]))
    pend = [b.submit(np.stack([caps[j], caps_b[j]])) for j in range(K - lag, K)]
    blob = a.b.export_channels([w for _, w in MOVED])
    b.b.import_channels([g for g, _ in MOVED], blob)
    b.b.switch_captures([g for g, _ in MOVED], [0, 0, 0])
    pend += [b.submit(np.stack([caps[j], caps_b[j]])) for j in range(K, K + 2)]
    b.b.wait(stream=b.s)
    torch.cuda.synchronize()
    slots = [g for g, _ in MOVED]
    for j, p in zip(range(K - lag, K + 2), pend):
        audio = p[1][:, :p[2]].cpu().numpy()
        for c in range(C8):
            if j >= K and c in slots:
                assert _same_audio(audio[c], ref["rec"][j]["audio"][dict(MOVED)[c]]), (j, c)
            else:
                assert _same_audio(audio[c], ref_b["rec"][j]["audio"][c]), (j, c)
    a.close()
    b.close()


@pytest.mark.parametrize("how", ["extra_call", "other_size"])
def test_clock_rule(pkg, caps, caps_b, how):
    """B has had one call more than A, or one call of another size: the import is refused with FMD_ERR_STATE naming
    the first differing word, nothing is queued, and B's later calls equal those of B without the attempt.  (The
    buffer parity alone: test_clock_rule_buffer_parity_alone.)"""
    a = Run(pkg)
    for j in range(4):
        a.call(caps[j])
    blob = a.b.export_channels([0, 1, 5])
    a.close()

    def feed(r, j):
        blk = np.stack([caps[j], caps_b[j]])
        if how == "other_size" and j == 3:
            blk = blk[:, :N]  # half the samples
        return r.call(blk)

    upto = 5 if how == "extra_call" else 4
    runs = [Run(pkg, shifts=SHIFTS_B, cmap=[1] * C8, n_cap=2) for _ in range(2)]
    for r in runs:
        for j in range(upto):
            feed(r, j)
    with pytest.raises(pkg.FmdError, match=FMD_ERR_STATE) as e:
        runs[0].b.import_channels([6, 2, 3], blob)
    assert "first in" in str(e.value) and ("if_pos" in str(e.value) or "lut_idx" in str(e.value)), str(e.value)
    for j in range(upto, upto + 2):
        _assert_same_call(feed(runs[0], j), feed(runs[1], j), j)
    with pytest.raises(pkg.FmdError, match="twice"):
        runs[0].b.import_channels([1, 2, 1], blob)
    with pytest.raises(pkg.FmdError, match="list names"):
        runs[0].b.import_channels([1, 2], blob)
    for r in runs:
        r.close()


def _fnv1a64(data):
    h = 0xcbf29ce484222325
    for x in data:
        h = ((h ^ x) * 0x100000001b3) & 0xffffffffffffffff
    return h


def _with_call_index_plus(blob, d):
    """the blob with d added to its clock's call index and nothing else changed: the field is 32 bits at byte 92 of
    the header (StateHeader in csrc/fmd_batch_state.inc.hpp: 64 bytes in front of the clock, the call index its eighth
    word), the checksum the header's last 8 of 144 bytes, FNV-1a 64 over the whole blob with that field zero"""
    b = bytearray(blob)
    assert _fnv1a64(bytes(b[:136]) + bytes(8) + bytes(b[144:])) == int.from_bytes(b[136:144], "little")
    ci = int.from_bytes(b[92:96], "little")
    b[92:96] = (ci + d).to_bytes(4, "little")
    b[136:144] = bytes(8)
    b[136:144] = _fnv1a64(bytes(b)).to_bytes(8, "little")
    return bytes(b), ci


def test_clock_rule_buffer_parity_alone(pkg, caps, caps_b, ref):
    """A difference of the buffer parity alone is refused, not placed: a blob of A whose call index is 2 more than
    B's, every other word of the clock equal (the blob's header edited, its checksum made right again), gives
    FMD_ERR_STATE naming call_index and nothing is queued.  The parity that counts is the call index mod 4 (the
    serial stage keeps the stereo flag per call index mod 4): the same blob with 4 added is taken, and the slots
    then are A's channels continuing, with B's own call indices."""
    a, b = _run_a_and_b(pkg, caps, caps_b, 6)
    blob = a.b.export_channels([w for _, w in MOVED])
    plus2, ci = _with_call_index_plus(blob, 2)
    assert ci == 6
    with pytest.raises(pkg.FmdError, match=FMD_ERR_STATE) as e:
        b.b.import_channels([g for g, _ in MOVED], plus2)
    assert "first in call_index" in str(e.value), str(e.value)
    plus4, _ = _with_call_index_plus(blob, 4)
    b.b.import_channels([g for g, _ in MOVED], plus4)
    b.b.switch_captures([g for g, _ in MOVED], [0, 0, 0])
    for j in range(6, 9):
        _assert_same_call(b.call(np.stack([caps[j], caps_b[j]])), ref["rec"][j], j, MOVED)
    a.close()
    b.close()


def test_single_decoder_save_and_load(pkg, oracle, fmsig):
    """FmDecoder on the stream of tests/golden/stereo_rds_2p4M.npz: SaveState behind block 9, LoadState into a new
    decoder, and the rest of the stream equals the oracle decoder's -- audio, getters, UECP frames."""
    import os
    from __graft_entry__ import ROOT
    g = np.load(os.path.join(ROOT, "tests", "golden", "stereo_rds_2p4M.npz"))
    fs, dn, nblk = float(g["fs"]), int(g["D"]), min(int(g["nblk"]), 16)
    p = fmsig.default_params(fs, noise_sigma=float(g["noise"]), seed=int(g["seed"]))
    o = oracle.OracleDecoder(fs, -0.15 * fs, 48000.0, 15000.0, dn)
    dec = pkg.FmDecoder(fs, -0.15 * fs, 48000.0, 15000.0, dn)
    frames = []
    for blk in range(nblk):
        iq = fmsig.u8_to_f32(fmsig.generate_u8(p, blk * N, N))
        want = o.process_stream(iq)
        if blk == 9:
            blob = dec.SaveState()
            frames = dec.sink.frames.get(0, [])
            dec.close()
            dec = pkg.FmDecoder(fs, -0.15 * fs, 48000.0, 15000.0, dn)
            dec.LoadState(blob)
        assert _bits(dec.ProcessStream(iq.view(np.complex64)), want), blk
        so = o.status()
        assert dec.StereoDetected() == bool(so.stereo), blk
        assert np.float32(dec.GetPilotLevel()) == np.float32(so.pilot_level), blk
        assert np.float32(dec.GetInterfaceLevel()) == np.float32(so.if_level), blk
    assert frames + dec.sink.frames.get(0, []) == o.uecp_frames()
    assert len(dec.sink.frames.get(0, [])) > 0
    dec.close()
