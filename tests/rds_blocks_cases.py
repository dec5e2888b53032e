"""The captures and streams the block-observation tests share (helper, not a conftest): built once per process, the
oracle run once per (capture, shift) stream and left unchanged.

Geometry: 2.4 MS/s, downsample 11, tuner table 24 -- shift k tunes k * 100 kHz.  A capture holds station A at
-700 kHz (shift 7; default_params(2.4e6, f_offset=-700e3, amp=0.3, seed=91, pi=0x7011, ps="LOUD") at a given noise
level) and station B at +300 kHz (shift -3), which sends the "all_types" group schedule: version-B groups, so that
offset word C' is tested.  Shift 2 is an empty step of every capture.  One capture is noise only.
"""
import numpy as np

import rds_sync_spec as spec  # (tests/ is on sys.path: pytest's rootdir-relative import of the test modules)

FS, D, TABLE = 2.4e6, 11, 24
N = 65536
SHIFT_A, SHIFT_B, SHIFT_EMPTY = 7, -3, 2
SIGMAS = (0.004, 0.15, 0.20)          # captures 0, 1, 2; capture 3: noise only
N_CAPTURES = 4
MIXED_CALLS = 150
# 60 ragged calls: 88 and 300 samples are RDS rows of 1 and 3 samples, the others no multiple of the 32-sample tile
RAGGED = [65536, 88, 300, 8192, 40000, 1001, 65536, 12345, 88, 20000] * 6
# the (capture, shift) streams of the mixed-lane test: at most 8
MIXED_STREAMS = [(0, SHIFT_A), (1, SHIFT_A), (2, SHIFT_A), (0, SHIFT_B), (2, SHIFT_B), (3, SHIFT_A), (0, SHIFT_EMPTY),
                 (2, SHIFT_EMPTY)]

_CACHE = {}


def station_a(fmsig, sigma):
    return fmsig.default_params(FS, f_offset=-700e3, amp=0.3, seed=91, pi=0x7011, ps="LOUD", noise_sigma=sigma)


def _sizes(name):
    return [N] * MIXED_CALLS if name == "mixed" else list(RAGGED)


def captures(fmsig, name):
    """[call][N_CAPTURES, 2 n] float32 IQ: the captures of stream set `name` ("mixed": 150 calls of 65 536 samples;
    "ragged": the 60 calls of RAGGED)"""
    key = ("cap", name)
    if key not in _CACHE:
        pb = fmsig.default_params(FS, f_offset=300e3, amp=0.3, seed=17, noise_sigma=0.0)
        dbits = fmsig.sched_dbits(fmsig.group_schedule("all_types"))
        pn = fmsig.default_params(FS, amp=0.0, seed=5, noise_sigma=0.2)
        pa = [station_a(fmsig, s) for s in SIGMAS]
        out, start = [], 0
        for n in _sizes(name):
            b = fmsig.generate_f32_bits(pb, dbits, start, n)
            rows = [fmsig.generate_f32(p, start, n) + b for p in pa] + [fmsig.generate_f32(pn, start, n)]
            out.append(np.stack(rows).astype(np.float32))
            start += n
        _CACHE[key] = out
    return _CACHE[key]


def plain_020(fmsig, name="ragged", u8=False):
    """[call][2 n]: station A alone at noise_sigma 0.20 (the stream of the issue's table), float32 or RTL-SDR bytes"""
    key = ("plain", name, u8)
    if key not in _CACHE:
        p, out, start = station_a(fmsig, 0.20), [], 0
        for n in _sizes(name):
            out.append(fmsig.generate_u8(p, start, n) if u8 else fmsig.generate_f32(p, start, n))
            start += n
        _CACHE[key] = out
    return _CACHE[key]


def oracle_spec(oracle, blocks, shift, key, u8=False, resets=(), modes=None):
    """The spec (records, counters, groups) and per-call (audio, status) of an oracle decoder with tuner shift `shift`
    on `blocks`; resets: calls (0-based) with a Reset in front; modes: the observation mode of every call (default 2).
    Cached under `key`."""
    key = ("spec", key, int(shift), u8, tuple(resets), None if modes is None else tuple(modes))
    if key not in _CACHE:
        o = oracle.OracleDecoder(FS, 0.0, 48000.0, 15000.0, D, table_size=TABLE, tuning_shift=int(shift))
        s = spec.SyncSpec(0)
        audio = []
        for k, iq in enumerate(blocks):
            if k in resets:
                o.reset()
                s.reset_machine()
            a = o.process_stream_u8(iq) if u8 else o.process_stream(iq)
            t = o.taps()
            s.call(k + 1, t["rds_mf"], t["rds_sync"], 2 if modes is None else modes[k])
            audio.append(a.copy())
        _CACHE[key] = (s, audio, o.rds_groups())
        o.close()
    return _CACHE[key]


def mixed_spec(oracle, fmsig, cap, shift):
    blocks = [c[cap] for c in captures(fmsig, "mixed")]
    return oracle_spec(oracle, blocks, shift, ("mixed", cap))


def kinds(records):
    """{(state, status): count} of a record array"""
    out = {}
    for st, ss in zip(records["state"].tolist(), records["status"].tolist()):
        out[(st, ss)] = out.get((st, ss), 0) + 1
    return out
