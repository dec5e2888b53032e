"""Non-finite, overflowing and denormal IQ: the comparison rule, the poison kinds, the capture layout and the oracle's
record of it (a plain helper module of tests/test_poison_cpu.py and tests/test_gpu_poison.py).

The rule (same_class) has no tolerance and leaves no element out: two floats agree when their 32 bits are equal or
when both are NaN -- sign and payload of a NaN are free, an invalid operation gives 0xFFC00000 on x86 and 0x7FC00000 on
the GPU --; infinities agree with their sign, finite values, the signs of zeros and denormals bit for bit; integers
must be equal outright.

The layout: G = 46 captures of one station each at 2.4 MS/s, D = 11, 48 kHz, four calls of SIZES samples (the third is
ragged).  Captures 0 .. 15 carry one Inf or NaN (alternating, in I and in Q) in call 1 at sample 30000 + 11 g, so that
the onset moves one baseband row per capture; 16 .. 23 at sample 11 (g - 16) of call 2, on top of the carried IF
history; 24 .. 31 at sample N - 1 - 11 (g - 24) of call 1, carried into the next call by the IF history; then an
overflowing burst, a stream times 1e30, one times 1e-39, one that fades through the denormal range into zeros, the six
degenerate kinds of tests/test_gpu_parity.py and four clean stations.  Channel c of a batch reads capture
(7 c + k) mod G."""
from collections import namedtuple

import numpy as np

FS, D, PCM, BW = 2.4e6, 11, 48000.0, 15000.0
OFFSET = -0.15 * FS
N = 65536
SIZES = (N, N, 40000, N)
STARTS = tuple(int(x) for x in np.concatenate([[0], np.cumsum(SIZES)[:-1]]))
TOTAL = int(sum(SIZES))
G = 46
K_VALUES = (0, 13)  # with 130 channels the last one reads capture 29 (poisoned) and 42 (clean)
STAGES = ("demod", "baseband", "pilot38", "mono_rs", "stereo_rs", "rds_lpf", "rds_pll", "rds_mf", "rds_sync")
DEGENERATE = ("silence", "dc", "noise", "clipped", "tone_at_carrier", "tiny")
POISONED = ("inf", "nan", "overflow")  # the kinds whose decoder turns NaN
KINDS = POISONED + ("big", "denormal", "fade") + DEGENERATE + ("clean",)
FADE_START, FADE_TAU = 30000, 800.0  # stream times exp(-t / 800 samples) from sample 30000 of call 0 on
BURST = 40

Capture = namedtuple("Capture", "kind base call sample part value")


# ---------------------------------------------------------------------------------------------------------------------
# the comparison rule

def _flat32(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.complex64:
        a = a.view(np.float32)
    return a


def mismatches(got, want):
    """indices (into the flattened arrays) of the elements that do not agree; None where shape or type differ"""
    g, w = _flat32(got), _flat32(want)
    if g.shape != w.shape or g.dtype != w.dtype:
        return None
    g, w = g.reshape(-1), w.reshape(-1)
    if g.dtype == np.float32:
        ok = (g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))
    else:
        assert g.dtype.kind in "iub", g.dtype  # integers: equal outright
        ok = g == w
    return np.flatnonzero(~ok)


def same_class(got, want):
    bad = mismatches(got, want)
    return bad is not None and bad.size == 0


def explain(got, want, n=4):
    """the first few disagreements as (index, got bits, wanted bits), for an assertion's message"""
    bad = mismatches(got, want)
    if bad is None:
        return "shape / type: %s %s against %s %s" % (np.shape(got), np.asarray(got).dtype, np.shape(want),
                                                       np.asarray(want).dtype)
    g, w = _flat32(got).reshape(-1), _flat32(want).reshape(-1)
    if g.dtype == np.float32:
        g, w = g.view(np.uint32), w.view(np.uint32)
    return "%d differ: %s" % (bad.size, [(int(i), hex(int(g[i])), hex(int(w[i]))) for i in bad[:n]])


def status_floats(s):
    """the four float getters of a status record (the oracle's or the product's) as float32"""
    return np.array([s.tuning_offset, getattr(s, "interface_level", getattr(s, "if_level", None)), s.baseband_level,
                     s.pilot_level], np.float32)


def status_stereo(s):
    return int(bool(getattr(s, "stereo_detected", getattr(s, "stereo", None))))


def same_status(got, want):
    """all five getters: the stereo flag equal, the four floats by same_class"""
    return status_stereo(got) == status_stereo(want) and same_class(status_floats(got), status_floats(want))


# ---------------------------------------------------------------------------------------------------------------------
# the kinds

def inject(stream, kind, position=0, part=0, value=None, seed=12345):
    """A copy of `stream` (interleaved float32 I, Q) with the poison of `kind`: `position` is the sample, `part` 0 = I,
    1 = Q, `value` the float an "inf" / "nan" puts there (default +Inf / NaN)."""
    x = np.array(stream, dtype=np.float32, copy=True)
    n = x.size // 2
    t = np.arange(n, dtype=np.float64)
    if kind == "clean":
        return x
    if kind == "inf":
        x[2 * position + part] = np.inf if value is None else value
    elif kind == "nan":
        x[2 * position + part] = np.nan if value is None else value
    elif kind == "overflow":  # 40 consecutive floats of +-3e38: the overflow happens inside the IF filter's sum
        x[2 * position:2 * position + BURST] = np.where(np.arange(BURST) % 3 == 0, -3e38, 3e38).astype(np.float32)
    elif kind == "big":
        x *= np.float32(1e30)
    elif kind == "denormal":
        x = (x.astype(np.float64) * 1e-39).astype(np.float32)
    elif kind == "fade":
        f = np.where(t >= position, np.exp(-np.maximum(t - position, 0.0) / FADE_TAU), 1.0)
        x = (x.astype(np.float64) * np.repeat(f, 2)).astype(np.float32)
    elif kind == "silence":
        x[:] = 0.0
    elif kind == "dc":
        x[0::2], x[1::2] = 0.3, 0.2
    elif kind == "noise":
        x[:] = (0.5 * np.random.default_rng(seed).standard_normal(2 * n)).astype(np.float32)
    elif kind == "clipped":
        x[0::2] = np.where((t // 7) % 2 == 0, 1.0, -1.0)
        x[1::2] = np.where((t // 5) % 2 == 0, 1.0, -1.0)
    elif kind == "tone_at_carrier":
        z = 0.5 * np.exp(2j * np.pi * (OFFSET / FS) * t)
        x[0::2], x[1::2] = z.real, z.imag
    elif kind == "tiny":
        z = 1e-30 * np.exp(2j * np.pi * (OFFSET / FS + 0.01 * np.sin(2 * np.pi * 1000 / FS * t)) * t)
        x[0::2], x[1::2] = z.real, z.imag
    else:
        raise ValueError("no such kind: %r" % (kind,))
    return x


def layout():
    """the G captures"""
    caps = []
    for g in range(32):
        kind = "inf" if g % 2 == 0 else "nan"
        value = (np.inf, -np.inf)[(g // 4) % 2] if kind == "inf" else np.nan
        part = (g // 2) % 2
        if g < 16:
            call, sample = 1, 30000 + 11 * g
        elif g < 24:
            call, sample = 2, 11 * (g - 16)
        else:
            call, sample = 1, SIZES[1] - 1 - 11 * (g - 24)
        caps.append(Capture(kind, g % 4, call, sample, part, value))
    caps.append(Capture("overflow", 0, 1, 30000, 0, None))
    caps.append(Capture("big", 1, 0, 0, 0, None))
    caps.append(Capture("denormal", 2, 0, 0, 0, None))
    caps.append(Capture("fade", 3, 0, FADE_START, 0, None))
    for i, kind in enumerate(DEGENERATE):
        caps.append(Capture(kind, i % 4, 0, 0, 0, None))
    for i in range(4):
        caps.append(Capture("clean", i, 0, 0, 0, None))
    assert len(caps) == G
    return caps


LAYOUT = layout()


def capture_of(c, k):
    return (7 * c + k) % G


def capture_map(C, k):
    return np.array([capture_of(c, k) for c in range(C)], np.uint32)


def base_streams(fmsig, fs=FS, total=TOTAL, n=4):
    """n stereo + RDS stations at the tuned frequency, `total` samples each (generated once per process)"""
    key = (fs, total, n)
    if key not in _cache:
        _cache[key] = [fmsig.generate_f32(fmsig.default_params(fs, noise_sigma=0.01, seed=501 + i, pi=0x7100 + i,
                                                               ps="POISON%d" % i, f_left=400.0 + 170 * i), 0, total)
                       for i in range(n)]
    return _cache[key]


_cache = {}


def captures(fmsig):
    """[G, 2 TOTAL] float32: the captures of the layout"""
    if "captures" not in _cache:
        base = base_streams(fmsig)
        rows = np.empty((G, 2 * TOTAL), np.float32)
        for g, cp in enumerate(LAYOUT):
            rows[g] = inject(base[cp.base], cp.kind, STARTS[cp.call] + cp.sample, cp.part, cp.value, seed=900 + g)
        rows.setflags(write=False)
        _cache["captures"] = rows
    return _cache["captures"]


def call_rows(rows, k):
    """what call k reads of captures `rows`: [.., 2 n] float32"""
    return rows[..., 2 * STARTS[k]:2 * (STARTS[k] + SIZES[k])]


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's record

def new_oracle(oracle, fs=FS, d=D, **kw):
    return oracle.OracleDecoder(fs, OFFSET / FS * fs, PCM, BW, d, **kw)


def run_oracle(oracle, stream, sizes, resets=(), fs=FS, d=D, taps=True, **kw):
    """One decoder over `stream` cut into calls of `sizes`, reset() in front of every call listed in `resets`: a record
    {audio, status, taps, groups, frames} per call."""
    o = new_oracle(oracle, fs, d, **kw)
    out, pos, ng, nf = [], 0, 0, 0
    for k, n in enumerate(sizes):
        if k in resets:
            o.reset()
        audio = o.process_stream(stream[2 * pos:2 * (pos + n)])
        pos += n
        groups, frames = o.rds_groups(ng), o.uecp_frames(nf)
        ng, nf = ng + len(groups), nf + len(frames)
        st = o.status()
        rec = {"audio": audio, "status": st, "groups": [blk for _, blk in groups], "frames": frames}
        if taps:
            rec["taps"] = o.taps()
        out.append(rec)
    o.close()
    return out


def reference(oracle, fmsig):
    """rec[g][k]: the oracle's record of capture g in call k (one decoder per capture, run once per process)"""
    if "reference" not in _cache:
        rows = captures(fmsig)
        _cache["reference"] = [run_oracle(oracle, rows[g], SIZES) for g in range(G)]
    return _cache["reference"]


BORDER = 128  # samples: a poison this close to a call's border may turn the audio NaN exactly at the border


def audio_onset(audio):
    """(call, float) of the first non-finite audio float of a lineage, None where it stays finite"""
    for k, a in enumerate(audio):
        bad = np.flatnonzero(~np.isfinite(a))
        if bad.size:
            return k, int(bad[0])
    return None


def assert_not_vacuous(rec, caps=LAYOUT, sizes=SIZES):
    """Every poisoned lineage has a NaN onset the comparison can get wrong, and every clean one is finite throughout.
    rec[g][k]["audio"] as reference() returns it.

    A poison inside a call: the oracle's audio of that very call has at least one finite and at least one NaN float.
    A poison within BORDER samples of a call's border (captures 16 .. 31) may, and for the nearest ones does, turn the
    audio NaN exactly at the border: the first samples of a call reach the first audio frame at once, and the last ones
    only reach the next call's, through the IF history.  There the onset lies in the poison's call or at the first
    frame of the next one, and the two calls around it together hold finite and NaN floats.  In both cases everything
    before the onset is finite and nothing behind it is."""
    for g, cp in enumerate(caps):
        audio = [r["audio"] for r in rec[g]]
        if cp.kind not in POISONED:
            for k, a in enumerate(audio):
                assert np.isfinite(a).all(), ("a clean lineage is not finite", g, cp, k)
            continue
        on = audio_onset(audio)
        assert on is not None, ("a poisoned lineage stays finite", g, cp)
        k, f = on
        inside = BORDER <= cp.sample < sizes[cp.call] - BORDER
        if inside:
            assert k == cp.call and f > 0, ("the onset is not inside the poison's call", g, cp, on)
        else:
            assert k == cp.call or (k == cp.call + 1 and f == 0), ("the onset is not at the poison", g, cp, on)
            assert k > 0 and audio[k - 1].size > 0, ("nothing finite in front of the onset", g, cp, on)
        assert not np.isinf(audio[k]).any() and np.isnan(audio[k][f:]).all(), ("not NaN for good", g, cp, on)
        for j in range(k + 1, len(audio)):
            assert np.isnan(audio[j]).all(), ("not NaN for good", g, cp, j)


# ---------------------------------------------------------------------------------------------------------------------
# edits after the poison (tests/edit_model.py: its geometry, stations and shifts)

EDIT_TAPS = ("baseband", "mono_rs", "stereo_rs", "rds_lpf", "rds_pll", "rds_mf")
EDIT_C = 130
# who does what (batch 0; channel c reads capture 1 (an Inf in call 1) where c % 4 == 0, capture 3 (a NaN in call 1)
# where c % 4 == 2, and the clean capture 0 otherwise; capture 4 is clean up to a NaN in call 3, capture 2 the B side)
EDIT_ROLES = {
    "early_reset": [2, 6, 66],           # reset in front of call 1, before the poison: another ring origin from there
    "reset": [0, 2, 64, 128, 4, 6, 96],  # poisoned, reset in front of call 2 (ragged: the first four) or call 3 (full)
    "retune": [8, 68, 36, 100],          # poisoned, retuned: a new decoder
    "to_clean": [12, 72, 40, 104],       # poisoned, switched to the clean capture: the state stays
    "to_poison": [1, 65, 3, 67],         # clean, switched to capture 4 in front of call 2 / call 3
    "export": [16, 44],                  # poisoned, imported over the clean slots 2, 3 of batch 1 (calls 2 and 5)
    "import": [48, 20],                  # poisoned slots that take the clean slots 6, 5 of batch 1 (calls 3 and 4)
}
EDIT_TAPS_OF = [0, 2, 4, 6, 1, 3]  # (below 8: the driver reads the same slots' taps of both batches)


def edit_case(oracle, fmsig):
    """(script, streams, model, shifts, capture maps) of the edits after the poison: two batches, 130 and 8 channels,
    nine calls; every edit kind once in front of a ragged call (2 or 4) and once in front of a full one (3 or 5), a
    save / load of both batches with their poisoned slots in front of call 6, a whole-batch reset of both in front of
    call 7.  Built once per process."""
    if "edit" in _cache:
        return _cache["edit"]
    import edit_model as em
    sizes = [N, N, 40000, N, 40000, N, N, N, N]
    start = [int(x) for x in np.concatenate([[0], np.cumsum(sizes)])]
    main = em.main_streams(fmsig, start[-1], two=True)
    clean, bside = main.rows[0][:2 * start[-1]], main.rows[1][:2 * start[-1]]
    streams = em.Streams.from_arrays([clean, inject(clean, "inf", start[1] + 30000, 0), bside,
                                      inject(clean, "nan", start[1] + 30005, 1),
                                      inject(clean, "nan", start[3] + 20000, 0)])
    r = EDIT_ROLES
    L, O = em.LOUD, em.OTHER
    # (an export is refused while edits of its batch are pending, a load among them: a move comes first at its boundary,
    # one move a boundary, and the save / load steps have a boundary of their own)
    script = em._steps(
        N, (N, [("reset", r["early_reset"])]),
        (40000, [("move", [16], [2]), ("reset", [0, 2, 64, 128]), ("retune", [8, 68], [L, O]),
                 ("switch", [12, 72, 1, 65], [0, 0, 4, 4])]),
        (N, [("move", [6], [48], 1, 0), ("reset", [4, 6, 96]), ("retune", [36, 100], [O, L]),
             ("switch", [40, 104, 3, 67], [0, 0, 4, 4])]),
        (40000, [("move", [5], [20], 1, 0)]), (N, [("move", [44], [3])]),
        (N, [("save_load",), (1, "save_load")]), (N, [("reset_all",), (1, "reset_all")]), N)
    shifts = [[L if c % 8 < 6 else O for c in range(EDIT_C)], [L, O, L, O, L, L, O, L]]
    cmaps = [[(1, 0, 3, 0)[c % 4] for c in range(EDIT_C)], [0] * 8]
    model = em.Model(oracle, streams, script, shifts, cmaps, taps=EDIT_TAPS)
    _cache["edit"] = (script, streams, model, shifts, cmaps)
    return _cache["edit"]


# ---------------------------------------------------------------------------------------------------------------------
# single infinities at chosen places, any geometry (the IF stage's kernel forms, the ring resampler at 250 taps)

def first_output_sample(oracle, fs, d, order=0):
    """The sample index of a fresh decoder's first IF output (its newest sample; -1: the sample in front of the first
    call), found on the oracle alone: an Inf at sample 320 d + j reaches output 320 exactly while j is not beyond it."""
    key = ("pos", fs, d, order)
    if key not in _cache:
        o = new_oracle(oracle, fs, d, if_filter_order=order)
        n = 322 * d + o.if_taps().size
        o.close()
        pos = None
        for j in range(-d, d):
            x = np.zeros(2 * n, np.float32)
            x[2 * (320 * d + j)] = np.inf
            dem = run_oracle(oracle, x, [n], fs=fs, d=d, if_filter_order=order)[0]["taps"]["demod"]
            first = int(np.flatnonzero(~np.isfinite(dem.view(np.float32)))[0]) // 2
            assert first in (319, 320, 321), (first, j)
            if first == 320:
                pos = j
        assert pos is not None and -d <= pos < d - 1
        _cache[key] = pos
    return _cache[key]


def point_case(oracle, fmsig, fs, d, sizes, points, order=0):
    """(rows [len(points) + 1, 2 total], rec[g][k]): capture i is one station with an infinity (its sign and I / Q
    alternate) at points[i] = (call, sample); the last capture is the station itself."""
    key = ("points", fs, d, tuple(sizes), tuple(points), order)
    if key not in _cache:
        start = [int(x) for x in np.concatenate([[0], np.cumsum(sizes)])]
        base = base_streams(fmsig, fs, start[-1], 1)[0]
        rows = np.stack([inject(base, "inf", start[k] + s, i % 2, (np.inf, -np.inf)[(i // 2) % 2])
                         for i, (k, s) in enumerate(points)] + [base])
        rows.setflags(write=False)
        rec = [run_oracle(oracle, r, sizes, fs=fs, d=d, if_filter_order=order) for r in rows]
        _cache[key] = (rows, rec)
    return _cache[key]


# ---------------------------------------------------------------------------------------------------------------------
# the receiver's audio meter over a call's float audio (cRadioReceiver::SamplesMeanRMS, RadioReceiver.cpp:584-598 and
# :526-528, as oracle/fmd_oracle.c rx_samples_mean_rms has it): float sums in sample order, float quotient and root

def audio_meter(audio, level):
    """(mean, rms, level behind the call) as float32 of one call's interleaved audio and the level in front of it"""
    a = np.ascontiguousarray(audio, np.float32)
    n = np.float32(a.size)
    with np.errstate(invalid="ignore", over="ignore"):
        vsum = np.cumsum(a, dtype=np.float32)[-1]
        vsumsq = np.cumsum((a * a).astype(np.float32), dtype=np.float32)[-1]
        mean = np.float32(vsum / n)
        rms = np.float32(np.sqrt(np.float32(vsumsq / n)))
        new = np.float32(0.95 * float(np.float32(level)) + 0.05 * float(rms))
    return mean, rms, new
