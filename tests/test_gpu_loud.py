"""ITU-R BS.1770 loudness blocks from the audio tail (fmd_batch_set_loudness, include/fmd.h):
the loudness forms of the eight audio tails and the host's block bookkeeping, through device calls.

No tolerance anywhere: every collected record equals, on its uint32 view, tests/loud_spec.py -- the definition
restated in numpy float32 -- applied to the CPU oracle's float audio of the same stream (the models of
tests/edit_model.py: one oracle decoder per history).  Where the channel count is beyond the oracle's reach the expected
records are those of a small batch of the same process that is itself held against the specification in the same
test; never the output under test.  Geometry: 2.4 MS/s, D 11, 48 kHz (min_samples() == 88, about one audio frame per
50 samples)."""
import numpy as np
import pytest

import edit_model as em
import loud_spec as ls
import poison
from __graft_entry__ import load_package
from test_gpu_feed import frames_of
from test_gpu_reset_channels import FS, D, T, SHIFTS0, _params, _stations

pytestmark = pytest.mark.gpu

N = 65536
KEEP = "keep"
SHIFTS130 = [int(x) for x in np.resize(np.array(SHIFTS0[:4], np.int32), 130)]  # stereo, stereo, mono, nothing there
CMAP130 = [(c // 4) % 4 for c in range(130)]  # every shift on every capture within the first 16 channels
ON = {"loud": True}
OFF = {"loud": False}


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def four_captures(fmsig, total):
    """capture 0: the three stations of tests/test_gpu_reset_channels.py; 1: one stereo + RDS station; 2: a mono
    station where capture 0 has a stereo one and a stereo one where it has the mono one; 3: noise alone"""
    sets = [_stations(fmsig), em.stations_b(fmsig),
            [fmsig.mono_params(FS, f_offset=-700e3, amp=0.25, noise_sigma=0.004, seed=94),
             fmsig.default_params(FS, f_offset=100e3, amp=0.2, noise_sigma=0.004, seed=95, pi=0x7055, ps="THIRD")],
            [fmsig.mono_params(FS, f_offset=300e3, amp=1e-5, noise_sigma=0.02, seed=96)]]
    return em.Streams(fmsig, "loud4", sets, total)


_MODELS = {}


def model_audio(oracle, streams, script, shifts, cmaps, key):
    """want(k) -> [C, 2 A] float32: every slot's audio in call k from the oracle model of tests/edit_model.py"""
    if key not in _MODELS:
        _MODELS[key] = em.Model(oracle, streams, script, shifts, cmaps, taps=())
    m = _MODELS[key]

    def want(k):
        return np.stack([m.at(k, c)["audio"] for c in range(m.C[0])])
    return want


def spec_blocks(want, plan, Cn, bf, rows=None, fs=48000.0):
    """(all blocks of the script [blocks, Cn], blocks completed up to and including every call): the specification
    over the audio of the mode-1 calls alone"""
    m = ls.Meter(fs, Cn, bf)
    out, done = [np.zeros((0, Cn), ls.LOUD_BLOCK_DTYPE)], []
    for k, step in enumerate(plan):
        if step["loud"]:
            a = want(k)
            out.append(m.push(a[:Cn] if rows is None else a[rows]))
        done.append(sum(len(o) for o in out))
    return np.concatenate(out), done


def same_blocks(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = ls.bits(got), ls.bits(want)
    bad = np.argwhere(g != w)
    assert bad.size == 0, (what, len(bad), [(int(j), int(c), int(f), hex(g[j, c, f]), hex(w[j, c, f]))
                                            for j, c, f in bad[:6]])


def _status_tuple(b, c):
    s = b.status(c)
    vals = (s.tuning_offset, s.interface_level, s.baseband_level, s.pilot_level) + tuple(b.audio_level(c))
    return (s.stereo_detected, s.rds_state) + tuple(int(np.float32(v).view(np.uint32)) for v in vals)


def _apply(b, edit, st):
    import torch
    kind, a = edit[0], edit[1:]
    if kind == "reset":
        b.reset_channels(list(a[0]))
    elif kind == "reset_all":
        b.wait(stream=st)
        torch.cuda.synchronize()
        b.reset()
    elif kind == "retune":
        b.retune(list(a[0]), list(a[1]), captures=list(a[2]) if len(a) > 2 else None)
    elif kind == "switch":
        b.switch_captures(list(a[0]), list(a[1]))
    elif kind == "move":  # within the batch: export the sources, import them into the destinations
        b.wait(stream=st)
        torch.cuda.synchronize()
        b.import_channels(list(a[1]), b.export_channels(list(a[0])))
    elif kind == "save_load":  # the saved state loaded back into the running batch
        b.wait(stream=st)
        torch.cuda.synchronize()
        b.load_state(b.save_state())
    else:
        raise ValueError(kind)


class Run:
    """One batch with device buffers through a script ((samples, [edits in front of the call])).  plan[k]: {"loud":
    the meter's mode of call k, "pcm": np.int16 for FMD_PCM_S16, "sel": an audio selection (None: every channel, KEEP:
    as it is), "feed": np.int16 / np.float32 for a feed call}.  collect_at[k]: a collect behind call k with the run's
    lag.  Keeps every call's delivered rows and what every collect returned."""

    def __init__(self, pkg, shifts, streams, cmaps=None, bf=97, ring=512, mode=1, lag=0, debug=None, enable=False,
                 feed_div=0, set_first=True, batch=None):
        import torch
        self.pkg, self.torch = pkg, torch
        self.Cn, self.streams, self.cmaps, self.mode, self.lag = len(shifts), streams, cmaps, mode, lag
        self.bf, self.ring = bf, ring
        b = batch or pkg.Batch(_params(pkg), self.Cn, tuning_shifts=np.array(shifts, np.int32),
                               record_callbacks=False)
        if enable:
            b.enable_retune()
        for key, v in (debug or {}).items():
            b.debug_set(key, v)
        b.set_concurrency(mode)
        if cmaps is not None:
            b.set_capture_map(cmaps, streams.G)
        if feed_div:
            b.set_feed(feed_div)
        self.b = b
        self.st = torch.cuda.current_stream().cuda_stream
        self.a_stride = (b.max_audio_floats(N) + 7) // 8 * 8
        self.f_stride = (max(b.max_feed_samples(N), 1) + 7) // 8 * 8 + 8
        self.pos, self.k = 0, 0
        self.keep, self.calls, self.collected, self.status = [], [], [], []
        self.cur_mode = None

    def call(self, n, step, edits=(), collect=True, status=False):
        torch, b = self.torch, self.b
        for e in edits:
            _apply(b, e, self.st)
        if step.get("sel", KEEP) is not KEEP:
            b.select_audio(step["sel"])
        if step["loud"] != self.cur_mode:
            b.set_loudness(step["loud"], self.bf, self.ring)
            self.cur_mode = step["loud"]
            assert b.loudness() == int(step["loud"])
        x = self.streams.block(self.pos, n)
        self.pos += n
        if n % 2:  # rows start on a pair of IQ samples
            x = np.concatenate([x, np.zeros((x.shape[0], 2), x.dtype)], axis=1)
        d_iq = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        iq_stride = x.shape[1] // 2 if (self.streams.G > 1 or self.cmaps is not None) else 0
        s16 = step.get("pcm") is not None and np.dtype(step["pcm"]) == np.int16
        stride = self.a_stride  # (elements of the format: as many int16 as floats)
        out = torch.zeros((self.Cn, stride), dtype=torch.int16 if s16 else torch.float32, device="cuda")
        kw = {"pcm": np.int16} if s16 else {}
        feed = None
        if step.get("feed") is not None:
            f16 = np.dtype(step["feed"]) == np.int16
            feed = torch.zeros((self.Cn, self.f_stride), dtype=torch.int16 if f16 else torch.float32, device="cuda")
            r = b.process_device(d_iq.data_ptr(), iq_stride, n, out.data_ptr(), stride, self.st,
                                 fmt=self.pkg.FMD_IQ_F32, d_feed_ptr=feed.data_ptr(), feed_stride=self.f_stride,
                                 feed=step["feed"], **kw)
            nf, nfeed = r
        else:
            nf, nfeed = b.process_device(d_iq.data_ptr(), iq_stride, n, out.data_ptr(), stride, self.st,
                                         fmt=self.pkg.FMD_IQ_F32, **kw), 0
        self.keep.append(d_iq)
        self.calls.append((out, nf, feed, nfeed))
        if status:
            b.wait(stream=self.st)
            torch.cuda.synchronize()
            self.status.append([_status_tuple(b, c) for c in range(self.Cn)])
        if collect:
            self.collect()
        self.k += 1

    def collect(self, lag=None, channels=None, cap=4096):
        blocks, first, lost = self.b.collect_loudness(lag=self.lag if lag is None else lag, channels=channels, cap=cap,
                                                      stream=self.st, with_lost=True)
        self.collected.append((blocks, first, lost))
        return blocks, first, lost

    def finish(self, close=True):
        torch, b = self.torch, self.b
        b.wait(stream=self.st)
        torch.cuda.synchronize()
        self.collect(lag=0)
        self.rows = [(o[:, :nf].cpu().numpy(), None if f is None else f[:, :nfeed].cpu().numpy())
                     for o, nf, f, nfeed in self.calls]
        self.groups = np.sort(b.collect_rds_array(cap=1 << 18, stream=self.st, run_group_decoder=False),
                              order=["channel", "call_index"])
        self.clipped = b.pcm_clipped()
        if close:
            b.close()
        return self

    def blocks(self):
        """every collected block in order (the collects must join up: nothing lost)"""
        at = 0
        for blk, first, lost in self.collected:
            assert lost == 0 and first == at, (first, at, lost)
            at += len(blk)
        return np.concatenate([blk for blk, _, _ in self.collected])


def play(pkg, shifts, streams, script, plan, status=False, collect_every=1, **kw):
    r = Run(pkg, shifts, streams, **kw)
    for k, (n, edits) in enumerate(script):
        r.call(n, plan[k], edits, collect=(k + 1) % collect_every == 0, status=status)
    return r.finish()


# ---------------------------------------------------------------------------------------------------------------
# 1. wave edges, ragged calls, block boundaries everywhere

def ragged_sizes():
    """Twelve call sizes from min_samples() up: one-frame calls, calls of fewer frames than a tile, a call that ends
    exactly on a block boundary of 97 and the next that starts on one, and two full calls (13 blocks of 97 each)."""
    return [88, 150, 300, 3663, 1001, N, 8192, 171, 12345, 330, 40000, N]


@pytest.fixture(scope="module")
def ragged(pkg, oracle, fmsig):
    script = [(n, []) for n in ragged_sizes()]
    streams = four_captures(fmsig, em.total_samples(script))
    return script, streams, model_audio(oracle, streams, script, SHIFTS130, CMAP130, "ragged")


@pytest.mark.parametrize("bf", [97, 1000])
@pytest.mark.parametrize("Cn", [1, 63, 65, 130])
def test_ragged_calls_equal_the_specification(pkg, ragged, Cn, bf):
    script, streams, want = ragged
    plan = [ON] * len(script)
    r = play(pkg, SHIFTS130[:Cn], streams, script, plan, cmaps=CMAP130[:Cn], bf=bf, ring=512)
    w, done = spec_blocks(want, plan, Cn, bf)
    same_blocks(r.blocks(), w, (Cn, bf))
    for k, (a, _) in enumerate(r.rows):  # the audio beside the meter is the oracle's
        assert np.array_equal(a.view(np.uint32), want(k)[:Cn].view(np.uint32)), k
    # the stream holds what it was built for: calls that complete 0, 1 and many blocks, boundaries on the first and
    # the last frame of a call and on every residue of the 16-frame tile
    A = frames_of([n for n, _ in script])
    per_call = np.diff([0] + done)
    print("frames", A, "blocks per call", list(per_call))
    assert {0, 1} <= set(per_call) and per_call.max() >= (13 if bf == 97 else 1)
    assert len(w) == sum(A) // bf
    if bf == 97:
        g0 = np.concatenate([[0], np.cumsum(A)])
        ends = [(j * bf - 1 - g0[k]) for k in range(len(A)) for j in range(1, len(w) + 1)
                if g0[k] <= j * bf - 1 < g0[k + 1]]
        assert {int(e) % 16 for e in ends} == set(range(16))


def test_boundaries_on_the_first_and_last_frame_of_a_call(pkg, oracle, fmsig):
    """call sizes found by walking the host plan so that a block ends on the last frame of a call and the next block
    on the first frame of a later one"""
    from test_gpu_feed import walk
    bf, sizes, state, g = 97, [], (0, np.float32(0.0)), 0

    def extend(pred, start):
        nonlocal state, g
        for n in range(start, start + 6000):
            A, behind = walk(state, n)
            if A and pred(g, A):
                sizes.append(n)
                state, g = behind, g + A
                return
        raise AssertionError("no call size found")

    extend(lambda g0, A: (g0 + A) % bf == 0, 3000)          # ends on the last frame of a block
    extend(lambda g0, A: (g0 + A) % bf == bf - 1, 500)      # the next block lacks one frame ...
    extend(lambda g0, A: A == 1, 88)                        # ... which is a whole call
    extend(lambda g0, A: (g0 + A) % bf == 1, 4000)          # a block ends on this call's last frame but one
    extend(lambda g0, A: True, 9000)
    script = [(n, []) for n in sizes]
    streams = four_captures(fmsig, em.total_samples(script))
    want = model_audio(oracle, streams, script, SHIFTS130[:65], CMAP130[:65], ("edges", tuple(sizes)))
    plan = [ON] * len(script)
    r = play(pkg, SHIFTS130[:65], streams, script, plan, cmaps=CMAP130[:65], bf=bf, ring=512)
    w, done = spec_blocks(want, plan, 65, bf)
    same_blocks(r.blocks(), w, "edges")
    per_call = list(np.diff([0] + done))
    assert per_call[2] == 1 and frames_of(sizes)[2] == 1 and per_call[0] >= 1


def test_setup_refusals_and_defaults(pkg):
    b = pkg.Batch(_params(pkg), 2, tuning_shifts=np.array(SHIFTS0[:2], np.int32), record_callbacks=False)
    assert b.loudness() == 0 and b.loudness_block_frames() == 4800
    assert np.array_equal(b.loudness_coeffs().view(np.uint32), ls.design(48000.0).astype(np.float32).view(np.uint32))
    blocks, first = b.collect_loudness()
    assert blocks.shape == (0, 2) and first == 0
    b.set_loudness(False, 1000, 8)  # mode 0 fixes nothing
    b.set_loudness(True, 97, 16)
    assert b.loudness() == 1 and b.loudness_block_frames() == 97
    for args, word in (((True, 98, 0), b"a block is 97 frames"), ((False, 1000, 0), b"a block is 97 frames"),
                       ((True, 0, 32), b"the ring holds 16 blocks")):
        with pytest.raises(pkg.FmdError):
            b.set_loudness(*args)
        assert word in pkg.lib().fmd_last_error()
    b.set_loudness(True, 97, 16)
    b.set_loudness(True)
    b.set_loudness(False)
    assert b.loudness() == 0 and b.loudness_block_frames() == 97
    with pytest.raises(pkg.FmdError):
        b.collect_loudness(channels=(1, 2))
    b.close()


# ---------------------------------------------------------------------------------------------------------------
# 2. every tail form; the other outputs keep their bits

FORMS = {
    "f32": {},
    "s16": {"pcm": np.int16},
    "sel": {"sel": [64, 3, 129, 0, 77]},
    "empty_sel": {"sel": []},
    "feed": {"feed": np.int16},
    "s16_feed": {"pcm": np.int16, "feed": np.float32},
    "sel_feed": {"sel": [5, 64, 1], "feed": np.float32},
    "s16_sel_feed": {"pcm": np.int16, "sel": [128, 2, 65, 66], "feed": np.int16},
}


@pytest.fixture(scope="module")
def forms_case(pkg, oracle, fmsig):
    sizes = [8192, 3663, 300, N, 8191, 12345]
    script = [(n, []) for n in sizes]
    streams = four_captures(fmsig, em.total_samples(script))
    want = model_audio(oracle, streams, script, SHIFTS130, CMAP130, "forms")
    return script, streams, want, spec_blocks(want, [ON] * len(script), 130, 97)[0]


@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_tail_form_meters_every_channel_and_changes_nothing_else(pkg, forms_case, form):
    """The meter beside S16 audio, an audio selection, no audio rows at all and the feed: the blocks of every channel,
    selected or not, are those of the plain float call, and audio, feed, status, audio meter, RDS groups and clip
    counters keep the bits of the same calls without the meter."""
    script, streams, want, w = forms_case
    step = FORMS[form]
    first = dict(step)
    plan_on = [dict(first, loud=True)] + [dict({k: v for k, v in step.items() if k != "sel"}, loud=True)] * 5
    plan_off = [dict(p, loud=False) for p in plan_on]
    kw = dict(cmaps=CMAP130, bf=97, ring=512, feed_div=2 if "feed" in step else 0)
    on = play(pkg, SHIFTS130, streams, script, plan_on, status=True, **kw)
    off = play(pkg, SHIFTS130, streams, script, plan_off, status=True, **kw)
    same_blocks(on.blocks(), w, form)
    assert sum(len(b) for b, _, _ in off.collected) == 0
    for k in range(len(script)):
        for x, y in zip(on.rows[k], off.rows[k]):
            assert (x is None) == (y is None)
            if x is not None:
                assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (form, k)
        assert on.status[k] == off.status[k], (form, k)
    assert np.array_equal(on.groups, off.groups)
    assert np.array_equal(on.clipped, off.clipped)
    if "pcm" not in step and "sel" not in step:
        for k in range(len(script)):
            assert np.array_equal(on.rows[k][0].view(np.uint32), want(k).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------
# 3. calls in flight, splices, collect cadences, a ring that loses blocks

@pytest.fixture(scope="module")
def flight_case(pkg, oracle, fmsig):
    sizes = [N, 8192, 3663, N, 300, 8192, N, 88, N, 12345] + [8192, N, 40000, 150, N, 8192, 330, N, 1001, N]
    script = [(n, []) for n in sizes]
    streams = four_captures(fmsig, em.total_samples(script))
    return script, streams, model_audio(oracle, streams, script, SHIFTS130[:65], CMAP130[:65], "flight")


TOGGLE = [True, True, False, True, True, True, False, False, True, True] * 2


@pytest.mark.parametrize("how,mode,lag", [("default", 0, 0), ("default", 1, 0), ("default", 2, 1), ("default", 2, 2),
                                          ("default", 2, 3), ("split_post", 2, 2), ("lpf_late0", 2, 1),
                                          ("lpf_late1", 2, 2), ("lpf_late2", 2, 3)])
def test_twenty_calls_in_flight_with_splices(pkg, flight_case, how, mode, lag):
    """20 calls on every stream layout and concurrency, the mode toggled in front of some: a mode-0 call is a splice
    -- the blocks are the specification over the mode-1 calls' frames alone --, collected behind every call at the
    run's lag, and never a block of a call younger than the lag."""
    script, streams, want = flight_case
    debug = {"default": None, "split_post": {"split_post": 1}, "lpf_late0": {"lpf_late": 0},
             "lpf_late1": {"lpf_late": 1}, "lpf_late2": {"lpf_late": 2}}[how]
    plan = [{"loud": t} for t in TOGGLE]
    r = play(pkg, SHIFTS130[:65], streams, script, plan, cmaps=CMAP130[:65], bf=97, ring=512, mode=mode, lag=lag,
             debug=debug)
    w, done = spec_blocks(want, plan, 65, 97)
    same_blocks(r.blocks(), w, (how, mode, lag))
    at = 0
    for k, (blk, first, lost) in enumerate(r.collected[:-1]):  # the collect behind call k: calls 0 .. k - lag
        at += len(blk)
        assert at == (done[k - lag] if k >= lag else 0), (k, at)
    assert len(w) > 60 and done[2] == done[1] and done[7] == done[5]


@pytest.mark.parametrize("every,lag", [(1, 0), (2, 1), (3, 2), (5, 0), (20, 0)])
def test_a_ring_of_eight_loses_what_it_must_and_nothing_else(pkg, flight_case, every, lag):
    """ring_blocks 8 against calls of up to 13 blocks: the ring holds the last 8 blocks completed by the calls
    submitted so far; what a collect finds older than that is counted in `lost` and skipped, first_block says where
    the survivors start, and the survivors are exact."""
    script, streams, want = flight_case
    plan = [{"loud": t} for t in TOGGLE]
    r = Run(pkg, SHIFTS130[:65], streams, cmaps=CMAP130[:65], bf=97, ring=8, mode=2, lag=lag)
    w, done = spec_blocks(want, plan, 65, 97)
    taken, losses = 0, 0
    for k, (n, _) in enumerate(script):
        r.call(n, plan[k], collect=False)
        if (k + 1) % every == 0:
            blk, first, lost = r.collect()
            avail = done[k - lag] if k >= lag else 0
            oldest = min(avail, max(0, done[k] - 8))
            want_lost = max(0, oldest - taken)
            start = max(taken, oldest)
            assert (first, lost, len(blk)) == (start, want_lost, avail - start), (k, first, lost, len(blk))
            same_blocks(blk, w[start:avail], ("ring", k))
            taken, losses = avail, losses + lost
    r.finish()
    assert losses > 0 and taken > 0


def test_collect_takes_the_named_channels_and_respects_cap(pkg, flight_case):
    script, streams, want = flight_case
    plan = [ON] * 4
    r = Run(pkg, SHIFTS130[:65], streams, cmaps=CMAP130[:65], bf=97, ring=512)
    for k in range(4):
        r.call(script[k][0], plan[k], collect=False)
    w, done = spec_blocks(want, plan, 65, 97)
    a, first_a, _ = r.collect(channels=(60, 5), cap=7)
    b, first_b, _ = r.collect(channels=(0, 1), cap=4096)
    assert (first_a, len(a), first_b, len(b)) == (0, 7, 7, done[3] - 7)
    same_blocks(a, w[:7, 60:65], "five channels, cap 7")
    same_blocks(b, w[7:, 0:1], "one channel, the rest")
    r.finish()


# ---------------------------------------------------------------------------------------------------------------
# 4. edits of the running batch leave the meter alone

def test_edits_between_calls_leave_the_meter_alone(pkg, oracle, fmsig):
    """a reset, a reset of single channels, a retune, a capture switch and an import between calls: the decoders do what
    the model says, the meter's states, sums and frame count carry on over whatever audio comes"""
    script = [(8192, []), (3663, [("reset", [1, 64, 7])]), (8192, [("retune", [2, 33], [7, -1])]),
              (300, [("switch", [0, 5, 64], [1, 2, 3])]), (8192, [("move", [0, 3], [10, 40])]),
              (12345, [("reset_all",)]), (8192, [("retune", [4], [-5], [2])]), (8191, [])]
    streams = four_captures(fmsig, em.total_samples(script))
    Cn = 65
    model_script = [(n, [e if e[0] != "move" else ("move", e[1], e[2], 0, 0) for e in edits]) for n, edits in script]
    want = model_audio(oracle, streams, model_script, SHIFTS130[:Cn], CMAP130[:Cn], "edits")
    plan = [ON] * len(script)
    r = play(pkg, SHIFTS130[:Cn], streams, script, plan, cmaps=CMAP130[:Cn], bf=97, ring=512, enable=True)
    for k, (a, _) in enumerate(r.rows):
        assert np.array_equal(a.view(np.uint32), want(k).view(np.uint32)), ("the model and the batch disagree", k)
    same_blocks(r.blocks(), spec_blocks(want, plan, Cn, 97)[0], "edits")


def test_a_loaded_batch_starts_its_meter_from_zero(pkg, oracle, fmsig):
    """save / destroy / load into a new batch: no blob carries the meter -- the new batch's blocks are those of a meter
    that starts at +0 with the first call it hears, over the audio of the uninterrupted decoder"""
    sizes = [8192, 3663, 8192, 300, 8192]
    script = [(n, []) for n in sizes]
    streams = four_captures(fmsig, em.total_samples(script))
    Cn = 8
    want = model_audio(oracle, streams, script, SHIFTS130[:Cn], CMAP130[:Cn], "load")
    a = Run(pkg, SHIFTS130[:Cn], streams, cmaps=CMAP130[:Cn], bf=97, ring=512)
    for k in range(2):
        a.call(sizes[k], ON)
    a.finish(close=False)
    blob = a.b.save_state()
    a.b.close()
    b = Run(pkg, SHIFTS130[:Cn], streams, cmaps=CMAP130[:Cn], bf=97, ring=512)
    b.b.load_state(blob)
    assert b.b.loudness() == 0
    b.pos = a.pos
    for k in range(2, 5):
        b.call(sizes[k], ON)
    b.finish()
    same_blocks(a.blocks(), spec_blocks(want, [ON, ON], Cn, 97)[0], "before the save")
    for i, k in enumerate(range(2, 5)):
        assert np.array_equal(b.rows[i][0].view(np.uint32), want(k).view(np.uint32)), k
    m = ls.Meter(48000.0, Cn, 97)
    w = np.concatenate([m.push(want(k)) for k in range(2, 5)])
    same_blocks(b.blocks(), w, "behind the load")


# ---------------------------------------------------------------------------------------------------------------
# 5. special inputs

def test_a_capture_that_falls_silent_for_several_calls_stays_exact(pkg, oracle, fmsig):
    """Capture 0 turns to all zeros for four full calls.  The records stay exact across the silence.
    This decoder does not fall silent behind a silent capture: its FM loop free-runs, the audio settles at a constant
    of 1.4e-3 with rounding jitter, and the block sums settle near 1e-11 (oracle and specification over 90 silent
    calls).  Nor does any other input reach the meter with denormals: the audio's level follows the deviation, not the
    capture's amplitude (a capture scaled by 1e-30 gives the same audio), and a reset in front of the silence starts
    the free run again at 3.4.  So no record of this decoder holds a denormal, and this test does not claim to
    exercise them; that the kernels keep denormals is pinned at build level by
    tests/test_loud_cabi_cpu.py::test_the_loudness_kernels_keep_float_denormals."""
    sizes = [8192, N, N, N, N, 8192]
    total = sum(sizes)
    base = four_captures(fmsig, total)
    rows = [np.array(r[:2 * total], copy=True) for r in base.rows]
    rows[0][2 * 8192:2 * (8192 + 4 * N)] = 0.0  # capture 0: all zeros for four calls
    streams = em.Streams.from_arrays(rows)
    script = [(n, []) for n in sizes]
    Cn = 20
    want = model_audio(oracle, streams, script, SHIFTS130[:Cn], CMAP130[:Cn], "silent")
    plan = [ON] * len(script)
    r = play(pkg, SHIFTS130[:Cn], streams, script, plan, cmaps=CMAP130[:Cn], bf=1000, ring=512)
    w, _ = spec_blocks(want, plan, Cn, 1000)
    same_blocks(r.blocks(), w, "silent")
    z = w["z_l"][:, [c for c in range(Cn) if CMAP130[c] == 0]]
    print("block sums of a silent channel:", z[:, 0])
    assert (z[-1] < 1e-3 * z[0]).all()


def test_a_nan_capture_poisons_its_lanes_only(pkg, oracle, fmsig):
    """a NaN in capture 3: its lanes' sums turn NaN and stay, their peaks follow the rule (a NaN sample leaves the
    peak) -- the specification over the audio those lanes deliver --; the lanes beside them are exact against the
    oracle"""
    sizes = [8192, 8192, 3663, 8192]
    total = sum(sizes)
    base = four_captures(fmsig, total)
    rows = [np.array(r[:2 * total], copy=True) for r in base.rows]
    rows[3] = poison.inject(rows[3], "nan", position=8192 + 1000)
    streams = em.Streams.from_arrays(rows)
    script = [(n, []) for n in sizes]
    Cn = 65
    clean = [c for c in range(Cn) if CMAP130[c] != 3]
    dirty = [c for c in range(Cn) if CMAP130[c] == 3]
    clean_rows = [np.array(r, copy=True) for r in base.rows]
    want = model_audio(oracle, em.Streams.from_arrays(clean_rows), script, SHIFTS130[:Cn], CMAP130[:Cn], "nan-clean")
    plan = [ON] * len(script)
    r = play(pkg, SHIFTS130[:Cn], streams, script, plan, cmaps=CMAP130[:Cn], bf=97, ring=512)
    got = r.blocks()
    w, done = spec_blocks(want, plan, Cn, 97)
    same_blocks(got[:, clean], w[:, clean], "the lanes beside the NaN capture")
    m = ls.Meter(48000.0, len(dirty), 97)
    own = np.concatenate([m.push(r.rows[k][0][dirty]) for k in range(len(script))])
    same_blocks(got[:, dirty], own, "the NaN lanes against the rule")
    assert np.isnan(got["z_l"][done[1]:, dirty]).all() and np.isnan(got["z_r"][done[1]:, dirty]).all()
    assert not np.isnan(got["peak_l"]).any() and not np.isnan(got["peak_r"]).any()
    assert not np.isnan(got["z_l"][:done[0], dirty]).any()


# ---------------------------------------------------------------------------------------------------------------
# 6. scale: several waves of workgroups, sub-batches, a single decoder

def _small_and_big(pkg, fmsig, oracle, Cn, sizes, key):
    """the blocks of an 8-channel batch held against the specification, and the run of Cn channels on one capture whose
    channel c is channel c % 8 of it"""
    script = [(n, []) for n in sizes]
    streams = em.main_streams(fmsig, em.total_samples(script))
    want = model_audio(oracle, streams, script, SHIFTS0, None, key)
    plan = [ON] * len(script)
    small = play(pkg, SHIFTS0, streams, script, plan, bf=97, ring=512)
    w, done = spec_blocks(want, plan, 8, 97)
    same_blocks(small.blocks(), w, "the small batch")
    shifts = [int(x) for x in np.resize(np.array(SHIFTS0, np.int32), Cn)]
    return script, streams, plan, shifts, w, done


def test_4160_channels(pkg, oracle, fmsig):
    Cn = 4160
    script, streams, plan, shifts, w, _ = _small_and_big(pkg, fmsig, oracle, Cn, [8192, 300, 3663, 8192], "scale")
    big = play(pkg, shifts, streams, script, plan, bf=97, ring=512, collect_every=2)
    got = big.blocks()
    assert got.shape == (len(w), Cn)
    same_blocks(got, w[:, np.arange(Cn) % 8], "4160 channels")


def test_a_shell_of_16384_channels_stitches_its_sub_batches(pkg, oracle, fmsig):
    """two sub-batches: a collect of five channels across their border behind three calls, then every channel of the
    fourth call's blocks -- all of them against the small batch's records, which are held against the specification"""
    Cn = 16384
    script, streams, plan, shifts, w, done = _small_and_big(pkg, fmsig, oracle, Cn, [8192, 300, 8192, 8192], "shell")
    r = Run(pkg, shifts, streams, bf=97, ring=512)
    for k in range(3):
        r.call(script[k][0], plan[k], collect=False)
    blk, first, lost = r.collect(channels=(8190, 5))
    assert (first, lost, len(blk)) == (0, 0, done[2])
    same_blocks(blk, w[:done[2], (8190 + np.arange(5)) % 8], "across the sub-batches")
    r.call(script[3][0], plan[3], collect=False)
    blk, first, lost = r.collect()
    assert (first, lost) == (done[2], 0) and len(blk) == done[3] - done[2] >= 1
    same_blocks(blk, w[done[2]:, np.arange(Cn) % 8], "every channel of both sub-batches")
    r.finish()


def test_a_single_decoder_through_its_batch(pkg, oracle, fmsig):
    sizes = [8192, 3663, 8192]
    streams = em.main_streams(fmsig, sum(sizes))
    dec = pkg.FmDecoder(FS, -700e3, 48000.0, 15000.0, D)  # the loud stereo station
    ref = oracle.OracleDecoder(FS, -700e3, 48000.0, 15000.0, D)
    view = dec.batch_view()
    view.set_loudness(True, 97, 64)
    m, pos, got, w = ls.Meter(48000.0, 1, 97), 0, [], []
    for n in sizes:
        x = streams.row(0, pos, n)
        pos += n
        a = dec.ProcessStream(x.view(np.complex64))
        a_ref = ref.process_stream(x)
        assert np.array_equal(a.view(np.uint32), a_ref.view(np.uint32))
        w.append(m.push(a_ref[None, :]))
        got.append(view.collect_loudness()[0])
    same_blocks(np.concatenate(got), np.concatenate(w), "a single decoder")
    assert sum(len(g) for g in got) >= 4
    dec.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. the default block at two PCM rates

@pytest.mark.parametrize("rate", [44100.0, 48000.0])
def test_the_default_100_ms_block(pkg, oracle, fmsig, rate):
    """block_frames 0: round(fs / 10) frames.  As many full-size calls as two blocks need, two captures."""
    bf = ls.default_block_frames(rate)
    calls = int(np.ceil(2 * bf / (N / FS * rate))) + 1
    streams = em.main_streams(fmsig, calls * N, two=True)
    shifts, cmap = [7, -5, -1, 5], [0, 0, 0, 1]
    params = pkg.make_params(FS, 0.0, rate, 15000.0, D, table_size=T, if_filter_order=0)
    b = pkg.Batch(params, 4, tuning_shifts=np.array(shifts, np.int32), record_callbacks=False)
    r = Run(pkg, shifts, streams, cmaps=cmap, bf=0, ring=0, batch=b)
    assert b.loudness_block_frames() == bf
    assert np.array_equal(b.loudness_coeffs().view(np.uint32), ls.design(rate).astype(np.float32).view(np.uint32))
    refs = [oracle.OracleDecoder(FS, 0.0, rate, 15000.0, D, table_size=T, if_filter_order=0, tuning_shift=s)
            for s in shifts]
    m, w, pos = ls.Meter(rate, 4), [], 0
    for k in range(calls):
        a = np.stack([refs[c].process_stream(streams.row(cmap[c], pos, N)) for c in range(4)])
        pos += N
        w.append(m.push(a))
        r.call(N, ON)
    r.finish()
    w = np.concatenate(w)
    assert len(w) == 2 and m.bf == bf
    same_blocks(r.blocks(), w, rate)
    # and what the host arithmetic makes of them: the loudness of 200 ms of the loud stereo station
    import importlib
    loud = importlib.import_module(pkg.__name__ + ".loudness")
    l = loud.window(r.blocks()[:, 0], bf)
    print("rate %g: %.2f LUFS over two blocks" % (rate, l))
    assert -40.0 < l < 0.0 and abs(l - ls.window(w[:, 0], bf)) <= 1e-9


# ---------------------------------------------------------------------------------------------------------------
# 8. mutation: the comparison has teeth

def test_dropping_the_carried_sums_breaks_exactly_the_blocks_that_span_a_call_boundary(pkg, ragged):
    script, streams, want = ragged
    Cn, bf = 65, 97
    plan = [ON] * len(script)
    r = Run(pkg, SHIFTS130[:Cn], streams, cmaps=CMAP130[:Cn], bf=bf, ring=512)
    r.b.debug_loud_skip_carry(1)
    for k, (n, _) in enumerate(script):
        r.call(n, plan[k])
    r.finish()
    got = r.blocks()
    w, _ = spec_blocks(want, plan, Cn, bf)
    assert got.shape == w.shape
    wrong = (ls.bits(got) != ls.bits(w)).any(axis=(1, 2))
    g0 = np.cumsum(frames_of([n for n, _ in script]))[:-1]  # first frames of calls 1 .. 11
    spans = np.array([any(j * bf < g < (j + 1) * bf for g in g0) for j in range(len(w))])
    print("blocks", len(w), "that span a boundary", int(spans.sum()), "wrong", int(wrong.sum()))
    assert spans.sum() >= 5 and np.array_equal(wrong, spans)
