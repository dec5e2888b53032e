"""The cases of the output fuzz (helper, not a conftest; no torch): random geometries in the distribution of
tests/test_gpu_fuzz_geometry.py crossed with what a call can deliver -- audio F32 / S16, MPX, feed and channel IQ rows
in both formats, drawn per call --, a feed divisor and an RDS block mode per batch, a row selection per kind changed in
front of one call, and one edit (reset of a channel, save -> destroy -> load) in front of another.

`case(i)` is stratified by index: every axis cycles over its values with a period of its own and only the rest comes
from random.Random(BASE + i), so a small count still visits every value.  `expectations(case, oracle, fmsig)` runs the
CPU oracle alone and returns what the device must deliver for the checked channels (0, C / 2, C - 1), from definitions
that exist already: the oracle's audio and taps, feed_spec.s16 / mpx16 / FeedSpec, rds_sync_spec.SyncSpec.

Every channel c of a case plays station c % 3 at the tuned frequency, generated on the host (the same blocks go to the
oracle and, expanded to C rows, to the device).  In a shared case the three stations are three captures that every
channel reads through a capture map with one tuner shift, and a capture switch moves a checked channel to the next
capture."""
import os
import random

import numpy as np

import feed_spec as fs
import rds_sync_spec as spec

BASE = 4177
N = 65536
N_DEFAULT = 32
CALLS = 6
FS_LIST = [250e3, 400e3, 1.0e6, 1.2e6, 1.44e6, 1.8e6, 2.048e6, 2.4e6, 2.56e6, 2.88e6, 3.2e6, 5.0e6, 8.0e6, 10e6]
CIC = [(6.4e6, 1), (12e6, 1), (12e6, 2), (16.2e6, 3)]
CIC_AT = {5: 0, 13: 2, 18: 1, 27: 3}          # case index -> CIC geometry
BIG_AT = (11, 23)                             # the two cases of 1030 channels
ORDERS = [0, "4D", "16D", 2, 3, 7, 100, 257, 1000, 4096, 1000]   # period 11
TABLES = [0, 1, 7, 24, 100, 1000]
CHANNELS = [1, 3, 63, 65, 130]                # period 5
PCM = [44100.0, 48000.0, 96000.0]             # period 3
BW = [15000.0, 12000.0]                       # period 2
RDS_MODE = [2, 1, 0, 2, 1, 2, 0]              # period 7
EDITS = ["none", "reset", "save_load", "switch"]
SHAPES = ["none", "one", "second", "perm"]
KINDS = ("audio", "mpx", "feed", "ciq")
RICH_FS = [250e3, 400e3, 1.0e6]
SIGMAS = (0.004, 0.15, 0.20)                  # rds_blocks_cases.SIGMAS: stations 0, 1, 2 of a noisy case
FMT = (None, "f32", "s16")


def n_cases():
    return int(os.environ.get("FMD_FUZZ_OUTPUT_CASES", str(N_DEFAULT)))


def clipped(x):
    """samples whose rounded value the S16 conversion has to clamp (NaN is not one)"""
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(np.asarray(x, np.float32) * np.float32(32768))
        return (r > 32767) | (r < -32768)


def selection(shape, C, seed):
    """the channel list of a selection shape; None: no selection (one row per channel)"""
    if shape == "none":
        return None
    if shape == "one":
        return [C // 2]
    if shape == "second":
        return list(range(0, C, 2))
    p = list(range(C))
    random.Random(seed).shuffle(p)
    return p


def case(i):
    """calls[2] is None: the short call, fmd_batch_min_samples() of the geometry, which resolve() fills in"""
    r = random.Random(BASE + i)
    cic = i in CIC_AT
    rich = not cic and (i % 2 == 0 or i % 10 == 1)  # enough signal for RDS groups: a low IF rate, long calls
    if cic:
        fs_if, D = CIC[CIC_AT[i]]
        order = 0
    else:
        rates = RICH_FS if rich else FS_LIST
        fs_if = r.choice(rates)
        ds = [d for d in range(1, 56) if 180e3 <= fs_if / d <= 420e3]
        if i % 4 == 1:  # even D where the rate has one
            while not any(d % 2 == 0 for d in ds):
                fs_if = r.choice(rates)
                ds = [d for d in range(1, 56) if 180e3 <= fs_if / d <= 420e3]
            ds = [d for d in ds if d % 2 == 0]
        D = r.choice(ds)
        order = ORDERS[i % 11]
        order = 4 * D if order == "4D" else 16 * D if order == "16D" else order
    C = 1030 if i in BIG_AT else CHANNELS[i % 5]
    edit = EDITS[(i // 3) % 4]
    shared = edit == "switch" or i % 10 == 4  # three captures, every channel the same tuner shift
    table = TABLES[(i + i // 6) % 6]
    if shared and table == 0:
        table = 24
    u8 = i % 4 in (1, 2)
    mode = r.choice([0, 1, 2, 2, 2])
    lag = r.choice([0, 1]) if mode == 2 else 0
    us = r.random() < 0.25
    tune = round(r.uniform(-0.4, 0.4), 4)
    shift = r.randrange(-int(0.4 * table), int(0.4 * table) + 1) if shared else 0
    nmax = min(N, 32700 * D)
    lo = min(max(2000, 8 * max(order, 8 * D)), nmax)
    if C == 1030:
        nmax = min(nmax, max(lo, 16384))
    lo = nmax * 3 // 4 if rich else min(lo, nmax * 3 // 4)
    q = 8 * D if cic else 1  # (the CIC stage reads past an odd block: such calls are refused)

    def ragged():
        return r.randrange(lo, nmax + 1)
    calls = [nmax, ragged(), None, ragged(), nmax if r.random() < 0.5 else ragged(), ragged()]
    calls = [n if n is None else max(q, n // q * q) for n in calls]
    outs = [dict(audio=("f32", "s16")[(i + k + k // 2) % 2], mpx=FMT[(i + k) % 3], feed=FMT[(i + 2 * k + k // 3) % 3],
                 ciq=FMT[(i // 3 + k) % 3]) for k in range(CALLS)]
    sel = {kind: SHAPES[(i // (j + 1) + j) % 4] for j, kind in enumerate(KINDS)}
    return dict(seed=i, fs=fs_if, D=D, order=order, C=C, table=table, u8=u8, mode=mode, lag=lag, pcm=PCM[i % 3],
                bw=BW[i % 2], us=us, tune=0.0 if shared else tune, cic=cic, calls=calls, outs=outs,
                feed_div=(2, 3)[(i // 3) % 2], rds_mode=RDS_MODE[i % 7], sel=sel, sel_call=r.randrange(1, CALLS),
                edit=edit, edit_call=2 + i % 4, edit_channel=C // 2, loud=(i + i // 3) % 3 == 0, shared=shared,
                shift=shift, lo=lo, nmax=nmax, rich=rich)


def decoder(k, oracle, pcm=None):
    return oracle.OracleDecoder(k["fs"], k["tune"] * k["fs"], k["pcm"] if pcm is None else pcm, k["bw"], k["D"],
                                us_version=k["us"], table_size=k["table"], if_filter_order=k["order"],
                                tuning_shift=k["shift"] if k["shared"] else None)


def min_samples(k, oracle):
    """fmd_batch_min_samples() from the oracle's design: the smallest baseband length that leaves every stage of the
    RDS decimator a sample (and an 11-tap stage 20, a CIC stage an even count) and holds an audio frame, times D"""
    o = decoder(k, oracle)
    hb, step = o.rds_hb_lengths(), float(o.constants()["resamp_step"])
    o.close()
    m = 5
    while m < step + 1.0:
        m += 1
    while True:
        n, ok = m, True
        for ln in hb:
            if ln == 0:
                ok, n = ok and n >= 2 and n % 2 == 0, n // 2
            elif ln == 11:
                ok, n = ok and n >= 20, n // 2
            else:
                n = n // 2 if n < ln else (n + 1) // 2
        if ok and n >= 1:
            return m * k["D"]
        m += 1


def resolve(k, oracle):
    """the case with its call sizes final: call 2 is the smallest call the geometry takes (under a CIC stage the next
    multiple of 8 D), and call 3 leaves M = 63, 0 or 1 mod 64 (M = ceil((n - phase) / D), the phase from the calls
    before)"""
    if k["calls"][2] is not None:
        return k
    k = dict(k, calls=list(k["calls"]))
    q = 8 * k["D"] if k["cic"] else 1
    smallest = min_samples(k, oracle)
    k["calls"][2] = -(-smallest // q) * q
    if not k["cic"]:
        D = k["D"]
        phase = -sum(k["calls"][:3]) % D
        m = max(k["calls"][3] // D // 64 * 64, 64) + (63, 0, 1)[k["seed"] % 3]
        n = (m - 1) * D + phase + 1
        if k["lo"] <= n <= k["nmax"]:
            k["calls"][3] = n
    # the loop back through channel IQ rows: where fmd_batch_baseband_limits takes every call's M (at least the
    # smallest call's, at most the largest block's, even under a CIC stage); of those every second case, and not the
    # two of 1030 channels
    k["loopback"] = k["seed"] % 2 == 1 and k["C"] <= 130 and all(
        smallest // k["D"] <= m <= -(-N // k["D"]) and (not k["cic"] or m % 2 == 0) for m in baseband_lengths(k))
    return k


def baseband_lengths(k):
    """M of every call of a resolved case: the decimator's phase walked over the calls"""
    pos, out = 0, []
    for n in k["calls"]:
        m = (n - pos + k["D"] - 1) // k["D"]
        pos += m * k["D"] - n
        out.append(m)
    return out


def cases(n=None):
    return [case(i) for i in range(n_cases() if n is None else n)]


def case_id(k):
    outs = "".join("".join("-" if o[x] is None else o[x][0] for x in KINDS) + "." for o in k["outs"])
    return "%02d-%gM-D%d-o%d-C%d%s%s-m%d%s-pcm%g-bw%g%s-f%d-r%d-%s%d-%s-%s" % (
        k["seed"], k["fs"] / 1e6, k["D"], k["order"], k["C"], ("-shared%d" if k["shared"] else "-t%d") % k["table"],
        "-u8" if k["u8"] else "", k["mode"],
        "-lag1" if k["lag"] else "", k["pcm"] / 1e3, k["bw"] / 1e3, "-us" if k["us"] else "", k["feed_div"],
        k["rds_mode"], k["edit"], k["edit_call"], "loud" if k["loud"] else "noisy", outs[:-1])


def checked(k):
    return sorted({0, k["C"] // 2, k["C"] - 1})


def stations(k, fmsig):
    """the three stations of a case (channel c plays station c % 3; in a shared case capture j holds station j),
    where the tuner looks: over-deviated and loud (S16 audio, feed and MPX saturate), or noise raised on stations /
    captures 1 and 2 (corrected and failed RDS blocks)"""
    at = -k["shift"] * k["fs"] / k["table"] if k["shared"] else k["tune"] * k["fs"]
    if k["loud"]:
        return [fmsig.default_params(k["fs"], f_offset=at, noise_sigma=0.005, dev=150e3, seed=300 + j,
                                     pi=0x6100 + j) for j in range(3)]
    # (the noise of rds_blocks_cases' station -- amp 0.3 at 2.4 MS/s -- at the same density per Hz at this rate)
    return [fmsig.default_params(k["fs"], f_offset=at, amp=0.3, noise_sigma=SIGMAS[j] * (k["fs"] / 2.4e6) ** 0.5,
                                 seed=300 + j, pi=0x6100 + j) for j in range(3)]


def blocks(k, fmsig):
    """[call][3, 2 n]: the stations' IQ of every call of a resolved case, float32 or RTL-SDR bytes"""
    ps, out, pos = stations(k, fmsig), [], 0
    for n in k["calls"]:
        out.append(np.stack([(fmsig.generate_u8 if k["u8"] else fmsig.generate_f32)(p, pos, n) for p in ps]))
        pos += n
    return out


def selections(k):
    """per call and row kind: the channel list in force (None: one row per channel)"""
    return [{kind: selection(k["sel"][kind], k["C"], k["seed"]) if c >= k["sel_call"] else None for kind in KINDS}
            for c in range(CALLS)]


def capture_of(k, c, j):
    """the capture (station) channel c reads in call j"""
    moved = k["edit"] == "switch" and c == k["edit_channel"] and j >= k["edit_call"]
    return (c % 3 + 1) % 3 if moved else c % 3


def feed_taps(k, oracle):
    f = np.float32(k["pcm"])
    fo = np.float32(f / np.float32(k["feed_div"]))
    return oracle.design_lp_kaiser(1.0, 60.0, float(np.float32(0.425) * fo), float(np.float32(0.575) * fo), float(f))


def expectations(k, oracle, fmsig, pcm=None, clip_all=False, feed_late=0):
    """{"case": the resolved case, "taps": feed taps, "ch": {c: {"calls": [per call: audio (in the call's format),
    n_audio, mpx, ciq, feed (in their formats, None where the call has none), frames, M, g0], "clip", "groups",
    "uecp", "records", "quality", "quality_saved", "status", "spec_groups"}}}.

    Edits: a reset is reset() of that decoder (feed and counters are the slot's and go on); after a switch the same
    decoder reads the other capture's block; a save, destroy and load into a new batch changes nothing in the decoder
    and the clip count, and the new batch's feed history and reception counters start at zero.
    pcm / clip_all / feed_late: wrong expectations for the harness's own test (another PCM rate, a clip count over
    every call, a feed that starts counting a frame late)."""
    k = resolve(k, oracle)
    taps = feed_taps(k, oracle)
    blks = blocks(k, fmsig)
    sels = selections(k)
    out = {"case": k, "taps": taps, "ch": {}}
    for c in checked(k):
        o = decoder(k, oracle, pcm)
        feed = fs.FeedSpec(taps, k["feed_div"])
        if feed_late:
            feed.x = np.zeros((1, feed_late), np.float32)
        sync = spec.SyncSpec(c)
        calls, clip, saved = [], 0, None
        for j, n in enumerate(k["calls"]):
            if j == k["edit_call"] and k["edit"] == "reset" and c == k["edit_channel"]:
                o.reset()
                sync.reset_machine()
            if j == k["edit_call"] and k["edit"] == "save_load":
                saved = sync.quality()
                sync.q = dict.fromkeys(spec.QUALITY_FIELDS, 0)
                feed = fs.FeedSpec(taps, k["feed_div"])
            x = blks[j][capture_of(k, c, j)]
            a = o.process_stream_u8(x) if k["u8"] else o.process_stream(x)
            t = o.taps()
            sync.call(j + 1, t["rds_mf"], t["rds_sync"], k["rds_mode"])
            w = k["outs"][j]
            e = dict(frames=a.size // 2, M=t["baseband"].size, g0=feed.g, n_audio=a.size, mpx=None, ciq=None, feed=None)
            e["audio"] = fs.s16(a) if w["audio"] == "s16" else a
            heard = sels[j]["audio"] is None or c in sels[j]["audio"]  # (the counter counts delivered samples)
            if (w["audio"] == "s16" and heard) or clip_all:
                clip += int(clipped(a).sum())
            if w["mpx"]:
                e["mpx_f32"] = t["baseband"]
                e["mpx"] = fs.mpx16(t["baseband"]) if w["mpx"] == "s16" else t["baseband"]
            if w["ciq"]:
                q = t["demod"]
                e["ciq"] = np.stack([fs.mpx16(q.real), fs.mpx16(q.imag)], axis=-1) if w["ciq"] == "s16" else q
            if w["feed"]:
                y = feed.push(a[None, :])[0]
                e["feed_f32"] = y
                e["feed"] = fs.s16(y) if w["feed"] == "s16" else y
            calls.append(e)
        s = o.status()
        out["ch"][c] = dict(calls=calls, clip=clip, groups=o.rds_groups(), uecp=o.uecp_frames(),
                            spec_groups=list(sync.groups),
                            records=sync.records_array(), quality=sync.quality(), quality_saved=saved,
                            status=(bool(s.stereo), s.if_level, s.baseband_level, s.pilot_level, s.tuning_offset))
        o.close()
    return out
