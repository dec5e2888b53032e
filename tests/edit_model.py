"""Scripts of per-channel edits of a running batch, their model on the CPU oracle and their driver on a batch.

A script is a list of steps (n_samples, [edits in front of this call]); the edits are

    ("reset", channels)                         fmd_batch_reset_channels
    ("reset_all",)                              fmd_batch_reset
    ("retune", channels, shifts[, captures])    fmd_batch_retune_channels[_to]
    ("switch", channels, captures)              fmd_batch_switch_captures
    ("move", src_channels, dst_channels)        export from batch 0, import into batch 1 ([, src_batch, dst_batch])
    ("save_load",)                              save_state, destroy the batch, load_state into a fresh one

and an edit whose first element is an integer is that batch's (default: batch 0).  Every batch of a script receives
every call, so their clocks stay equal.

The model (Model) follows the contracts of include/fmd.h with one oracle decoder lineage per distinct history: a reset
is reset() on the decoder, a retune a new decoder with that shift fed float zeros of the actual size of every earlier
call (reset() wherever the batch had a whole-batch reset) that reads the slot's capture from then on, a switch the same
decoder reading another capture, a move the decoder following the slot, save / load nothing.  The histories form a
tree (a node per call: reset in front of it or not, what it read); slots with the same history share its nodes, and one
decoder runs per leaf, so a batch of any size costs a handful of decoders.

The driver (Driver) plays the same script on batches: host-buffer calls, device calls one at a time, or device calls
at concurrency 2 with the outputs consumed `lag` calls late.  The stations, shifts, tuner table and helpers are those of
tests/test_gpu_reset_channels.py; the batches are the Run objects of tests/test_gpu_state.py."""
from collections import namedtuple

import numpy as np

from test_gpu_reset_channels import (FS, D, T, N, RDS_TAPS, SHIFTS0, _bits, _oracle, _params, _shift_of, _stations,
                                     _status_equal)

# call sizes at which the 2.4 MS/s, D = 11 geometry takes another path (tests/test_gpu_geometries.py:
# test_short_calls_bit_exact), the RDS rows they give being 1 (88 .. 150), 2, 3, 11, 42 (3663: the last below the
# matched filter's 44 taps), 94, 141 and 455
EDGES = [88, 89, 97, 100, 150, 170, 171, 300, 330, 1001, 3662, 3663, 8191, 8192, 12345, 40000]
T_LPF, T_MF = 75, 44  # taps of the RDS low-pass and the matched filter at this geometry
LOUD, OTHER, MONO, BSIDE = _shift_of(-700e3), _shift_of(500e3), _shift_of(100e3), _shift_of(-500e3)

Geometry = namedtuple("Geometry", "fs d t order", defaults=(FS, D, T, 0))
GEOM = Geometry()


def stations_b(fmsig, fs=FS):
    """the second capture: one stereo + RDS station at -500 kHz (batch B's of tests/test_gpu_state.py)"""
    return [fmsig.default_params(fs, f_offset=-500e3, amp=0.25, noise_sigma=0.004, seed=97, pi=0x7044, ps="BSIDE")]


def _to_u8(cap):
    """the capture as RTL-SDR byte pairs (as tests/test_gpu_state.py does it)"""
    return np.clip(np.round(cap * 127.5 + 127.5), 0, 255).astype(np.uint8)


class Streams:
    """G captures, each one continuous stream of `total` samples (the sum of its stations); row(g, pos, n) is what call
    reads of capture g.  The streams are generated once per process and name."""
    _cache = {}

    def __init__(self, fmsig, name, station_sets, total, u8=False):
        self.u8, self.G = u8, len(station_sets)
        self.rows = []
        for g, st in enumerate(station_sets):
            have = Streams._cache.get((name, g))
            if have is None or have.size < 2 * total:
                have = np.zeros(2 * total, np.float32)
                for p in st:
                    have += fmsig.generate_f32(p, 0, total)
                Streams._cache[(name, g)] = have
            if u8:
                if (name, g, "u8") not in Streams._cache or Streams._cache[(name, g, "u8")].size < 2 * total:
                    Streams._cache[(name, g, "u8")] = _to_u8(have)
                have = Streams._cache[(name, g, "u8")]
            self.rows.append(have)

    @classmethod
    def from_arrays(cls, rows):
        """the streams of given captures: interleaved float32 I, Q per capture (they may hold any float at all)"""
        s = cls.__new__(cls)
        s.u8, s.rows = False, [np.ascontiguousarray(r, dtype=np.float32) for r in rows]
        s.G = len(s.rows)
        return s

    def row(self, g, pos, n):
        r = self.rows[g][2 * pos:2 * (pos + n)]
        assert r.size == 2 * n, "the stream is shorter than the script"
        return r

    def block(self, pos, n):
        return np.stack([self.row(g, pos, n) for g in range(self.G)])


def main_streams(fmsig, total, u8=False, two=False):
    """capture 0: the three stations of tests/test_gpu_reset_channels.py; with `two`, capture 1: stations_b"""
    sets = [_stations(fmsig)] + ([stations_b(fmsig)] if two else [])
    return Streams(fmsig, "main", sets, total, u8)


def total_samples(script):
    return sum(n for n, _ in script)


def _norm(edit):
    """(batch, kind, arguments) of an edit"""
    if isinstance(edit[0], (int, np.integer)):
        return int(edit[0]), edit[1], tuple(edit[2:])
    return 0, edit[0], tuple(edit[1:])


class Model:
    """What every slot of every batch delivers in every call of a script, from oracle decoders alone."""

    def __init__(self, oracle, streams, script, shifts, cmaps=None, geom=GEOM, taps=RDS_TAPS, wrong_history=None):
        """shifts: the tuning shifts of one batch, or a list of them for several; cmaps: the capture of every channel
        likewise (None: capture 0).  wrong_history = n: a retuned decoder's earlier calls are zeros of n samples each
        instead of the real sizes (what the contract does NOT say; for showing that the sizes matter)."""
        if not isinstance(shifts[0], (list, tuple, np.ndarray)):
            shifts, cmaps = [shifts], [cmaps] if cmaps is not None else None
        self.oracle, self.streams, self.script, self.geom, self.tap_names = oracle, streams, script, geom, tuple(taps)
        self.wrong_history = wrong_history
        nb = len(shifts)
        self.C = [len(s) for s in shifts]
        shift = [[int(x) for x in s] for s in shifts]
        cap = [[int(x) for x in (cmaps[b] if cmaps is not None and cmaps[b] is not None else [0] * self.C[b])]
               for b in range(nb)]
        self.parent, self.info, self._index = [], [], {}
        node = [[-1] * self.C[b] for b in range(nb)]
        self.fresh = [[True] * self.C[b] for b in range(nb)]  # the slot's decoder began with a blank PS name here
        self.resets_all = [set() for _ in range(nb)]
        self.events = []  # (call, batch, kind, channels)
        self.at_ = []
        for k, (n, edits) in enumerate(script):
            pend = [[False] * self.C[b] for b in range(nb)]
            all_reset = [False] * nb
            for e in edits:
                b, kind, a = _norm(e)
                if kind == "reset":
                    for c in a[0]:
                        pend[b][c], self.fresh[b][c] = True, True
                    self.events.append((k, b, kind, list(a[0])))
                elif kind == "reset_all":
                    self.resets_all[b].add(k)
                    all_reset[b] = True
                    pend[b] = [True] * self.C[b]
                    self.fresh[b] = [True] * self.C[b]
                    self.events.append((k, b, kind, list(range(self.C[b]))))
                elif kind == "retune":
                    for i, c in enumerate(a[0]):
                        shift[b][c] = int(a[1][i])
                        node[b][c] = self._zero_path(b, shift[b][c], k)
                        pend[b][c], self.fresh[b][c] = all_reset[b], True
                        if len(a) > 2:
                            cap[b][c] = int(a[2][i])
                    self.events.append((k, b, "retune_to" if len(a) > 2 else kind, list(a[0])))
                elif kind == "switch":
                    for i, c in enumerate(a[0]):
                        cap[b][c] = int(a[1][i])
                    self.events.append((k, b, kind, list(a[0])))
                elif kind == "move":
                    sb, db = (a[2], a[3]) if len(a) > 2 else (0, 1)
                    took = [(node[sb][c], shift[sb][c], pend[sb][c]) for c in a[0]]
                    for c, (nd, sh, pe) in zip(a[1], took):
                        node[db][c], shift[db][c], pend[db][c], self.fresh[db][c] = nd, sh, pe, False
                    self.events.append((k, db, kind, list(a[1])))
                elif kind == "save_load":
                    self.events.append((k, b, kind, []))
                else:
                    raise ValueError("no such edit: %r" % (e,))
            for b in range(nb):
                for c in range(self.C[b]):
                    node[b][c] = self._child(node[b][c], k, pend[b][c], cap[b][c], shift[b][c])
            self.at_.append([list(node[b]) for b in range(nb)])
        self._evaluate()

    # -- the tree of histories
    def _child(self, parent, k, reset, src, shift):
        key = (parent, k, bool(reset), src, shift if parent < 0 else None)
        i = self._index.get(key)
        if i is None:
            i = len(self.parent)
            self._index[key] = i
            self.parent.append(parent)
            self.info.append((k, bool(reset), src, shift))
        return i

    def _zero_path(self, b, shift, k):
        """the history of a decoder created with `shift` that has received zeros in the calls 0 .. k - 1 and reset()
        wherever batch b had a whole-batch reset"""
        p = -1
        for i in range(k):
            p = self._child(p, i, i in self.resets_all[b], "z", shift)
        return p

    def _evaluate(self):
        needed = {i for call in self.at_ for batch in call for i in batch}
        has_child = set(self.parent)
        self.rec = {}
        pos = np.concatenate([[0], np.cumsum([n for n, _ in self.script])]).astype(np.int64)
        self.decoders = 0
        for leaf in sorted(needed - has_child):
            path = []
            i = leaf
            while i >= 0:
                path.append(i)
                i = self.parent[i]
            path.reverse()
            g = self.geom
            o = _oracle(self.oracle, self.info[path[0]][3], g.fs, g.d, g.t, g.order)
            self.decoders += 1
            ngroups = nframes = 0
            for i in path:
                k, reset, src, _ = self.info[i]
                n = self.script[k][0]
                if reset:
                    o.reset()
                if src == "z":
                    audio = o.process_stream(np.zeros(2 * (self.wrong_history or n), np.float32))
                elif self.streams.u8:
                    audio = o.process_stream_u8(self.streams.row(src, int(pos[k]), n))
                else:
                    audio = o.process_stream(self.streams.row(src, int(pos[k]), n))
                groups, frames = o.rds_groups(ngroups), o.uecp_frames(nframes)
                ngroups, nframes = ngroups + len(groups), nframes + len(frames)
                if i in needed and i not in self.rec:
                    t = o.taps()
                    self.rec[i] = {"audio": audio, "status": o.status(), "taps": {x: t[x] for x in self.tap_names},
                                   "rows": len(t["rds_mf"]), "groups": [blk for _, blk in groups], "frames": frames,
                                   "name": o.channel_name()}
            o.close()
        self.R = [self.rec[call[0][0]]["rows"] for call in self.at_]

    # -- what the tests ask
    def at(self, k, c, b=0):
        """the record of slot c of batch b in call k: audio, status, taps, the call's groups and frames, PS name"""
        return self.rec[self.at_[k][b][c]]

    def lineages(self, k, b=0):
        """{history node: [slots]} of batch b in call k"""
        out = {}
        for c, i in enumerate(self.at_[k][b]):
            out.setdefault(i, []).append(c)
        return out

    def one_per_lineage(self, b=0):
        """a smallest set of slots of batch b that shows every history node some slot of it is on in some call"""
        pick, seen = [], set()
        for k in range(len(self.script)):
            for i, slots in self.lineages(k, b).items():
                if i not in seen:
                    seen.add(i)
                    if not any(self.at_[k][b][c] == i for c in pick):
                        pick.append(slots[0])
        return sorted(set(pick))

    def phases(self, k, b=0):
        """batch b's RDS low-pass and matched-filter ring phases at the first sample of call k: the RDS rows since the
        batch's creation or last whole-batch reset, mod the tap counts"""
        since = max([r for r in self.resets_all[b] if r <= k], default=0)
        rows = sum(self.R[since:k])
        return rows % T_LPF, rows % T_MF

    def reset_report(self, follow=8):
        """[(call, batch, channels, (low-pass phase, matched-filter phase), rows of the `follow` calls from there)] of
        every per-channel reset"""
        return [(k, b, ch, self.phases(k, b), self.R[k:k + follow]) for k, b, kind, ch in self.events
                if kind == "reset"]

    def groups_around(self, c, k, b=0):
        """(groups slot c of batch b delivered in the calls before k, in the calls from k on)"""
        per_call = [len(self.at(j, c, b)["groups"]) for j in range(len(self.script))]
        return sum(per_call[:k]), sum(per_call[k:])


# ---------------------------------------------------------------------------------------------------------------------
# the driver

class Driver:
    """Plays a script on one or more batches and records what they deliver.

    mode "host": process_host / process_host_u8, one call at a time (the group decoder runs inside the call: frames
    and names, no groups); "device": process_device and collect_rds one call at a time; "flight": process_device at
    concurrency 2, waits and collect_rds `lag` calls late (audio, the groups with their call index, frames, names and
    the getters behind the last call)."""

    def __init__(self, pkg, streams, shifts, cmaps=None, mode="device", lag=0, geom=GEOM, enable=True, debug=None,
                 taps_of=(), tap_names=RDS_TAPS, keep_phase=False, status_of=None, callbacks=True):
        if not isinstance(shifts[0], (list, tuple, np.ndarray)):
            shifts, cmaps = [shifts], [cmaps] if cmaps is not None else None
        self.pkg, self.streams, self.mode, self.lag, self.geom = pkg, streams, mode, lag, geom
        if cmaps is None and streams.G > 1:
            cmaps = [[0] * len(s) for s in shifts]
        self.shifts, self.cmaps = shifts, cmaps
        self.kw = dict(enable=enable, debug=debug, taps=bool(taps_of), keep_phase=keep_phase, callbacks=callbacks)
        self.taps_of, self.tap_names, self.callbacks = list(taps_of), tuple(tap_names), callbacks
        self.status_of = status_of
        nb = len(shifts)
        self.units = [self._make(b) for b in range(nb)]
        self.frames = [{} for _ in range(nb)]
        self.names = [{} for _ in range(nb)]
        self.res = []
        self.pend = [[] for _ in range(nb)]
        self.groups = [[] for _ in range(nb)]  # "flight": (channel, call index, blocks) in collection order

    def _make(self, b):
        from test_gpu_state import Run
        g = self.geom
        cmap = self.cmaps[b] if self.cmaps is not None else None
        return Run(self.pkg, shifts=self.shifts[b], conc=2 if self.mode == "flight" else None,
                   cmap=cmap if self.streams.G > 1 else None, n_cap=self.streams.G,
                   params=_params(self.pkg, g.fs, g.d, g.t, g.order), **self.kw)

    def _pull(self, b):
        """move what the callbacks received since the last look into the per-slot lists"""
        if not self.callbacks:
            return
        u = self.units[b]
        for c, fr in u.b.sink.frames.items():
            if fr:
                self.frames[b].setdefault(c, []).extend(fr)
        u.b.sink.frames.clear()
        for c, nm in u.b.sink.names.log.items():
            if nm:
                self.names[b].setdefault(c, []).extend(nm)
        u.b.sink.names.log.clear()

    def _settle(self, b):
        """wait for every call of batch b and take its groups (what a save or a whole-batch reset needs first)"""
        import torch
        u = self.units[b]
        if self.mode == "host":
            return
        u.b.wait(stream=u.s)
        torch.cuda.synchronize()
        if self.mode == "flight":
            self.groups[b] += u.b.collect_rds(run_group_decoder=self.callbacks, stream=u.s)
        self._pull(b)

    def _edit(self, e):
        b, kind, a = _norm(e)
        u = self.units[b]
        if kind == "reset":
            u.b.reset_channels(list(a[0]))
        elif kind == "reset_all":
            self._settle(b)
            u.b.reset()
        elif kind == "retune":
            u.b.retune(list(a[0]), list(a[1]), captures=list(a[2]) if len(a) > 2 else None)
        elif kind == "switch":
            u.b.switch_captures(list(a[0]), list(a[1]))
        elif kind == "move":
            sb, db = (a[2], a[3]) if len(a) > 2 else (0, 1)
            blob = self.units[sb].b.export_channels(list(a[0]))
            self.units[db].b.import_channels(list(a[1]), blob)
        elif kind == "save_load":
            self._settle(b)
            blob = u.b.save_state()
            self._finish_pending(b)
            u.close()
            self.units[b] = self._make(b)
            self.units[b].b.load_state(blob)
        else:
            raise ValueError("no such edit: %r" % (e,))

    def _finish_pending(self, b):
        for k, (_, out, nf) in self.pend[b]:
            self.res[k][b]["audio"] = out[:, :nf].cpu().numpy()
        self.pend[b] = []

    def _status(self, u):
        chans = range(u.C) if self.status_of is None else self.status_of
        return {c: (u.b.status(c), u.b.status_call_index(c)) for c in chans}

    def _call(self, b, k, pos, n):
        import torch
        u = self.units[b]
        x = self.streams.block(pos, n)
        r = {}
        if self.mode == "host":
            shared = self.streams.G == 1
            x = x[0] if shared else x
            r["audio"] = u.b.process_host_u8(x, shared=shared) if self.streams.u8 else \
                u.b.process_host(x.view(np.complex64), shared=shared)
        else:
            if self.streams.G > 1 and n % 2:  # capture rows start on a pair of IQ samples: a stride of n + 1
                x = np.concatenate([x, np.zeros((x.shape[0], 2), x.dtype)], axis=1)
            p = u.submit(x[0] if self.streams.G == 1 else x, samples=n)
            if self.mode == "flight":
                self.pend[b].append((k, p))
                if k >= self.lag:
                    u.b.wait(stream=u.s, lag=self.lag)
                    self.groups[b] += u.b.collect_rds(run_group_decoder=self.callbacks, stream=u.s, lag=self.lag)
                return r
            u.b.wait(stream=u.s)
            torch.cuda.synchronize()
            r["audio"] = p[1][:, :p[2]].cpu().numpy()
            r["groups"] = u.b.collect_rds(run_group_decoder=self.callbacks, stream=u.s)
        r["status"] = self._status(u)
        r["taps"] = {c: {t: u.b.tap(t, c) for t in self.tap_names} for c in self.taps_of}
        self._pull(b)
        r["nframes"] = {c: len(f) for c, f in self.frames[b].items()}
        return r

    def play(self, script, upto=None):
        """runs the script (its calls [len(self.res), upto)) and returns the records: res[k][batch]"""
        first = len(self.res)
        pos = sum(n for n, _ in script[:first])
        for k in range(first, len(script) if upto is None else upto):
            n, edits = script[k]
            for e in edits:
                self._edit(e)
            self.res.append(None)
            self.res[k] = [None] * len(self.units)
            for b in range(len(self.units)):
                self.res[k][b] = self._call(b, k, pos, n)
            pos += n
        return self.res

    def finish(self):
        """waits for everything, completes the records of the calls in flight, closes the batches.  Returns the getters
        behind the last call per batch."""
        last = []
        for b, u in enumerate(self.units):
            self._settle(b)
            self._finish_pending(b)
            last.append(self._status(u))
            u.close()
        return last


# ---------------------------------------------------------------------------------------------------------------------
# comparisons (every one bitwise)

def frames_of_call(drv, res, k, c, b=0):
    """the UECP frames slot c of batch b received in call k of a serial run"""
    before = res[k - 1][b]["nframes"].get(c, 0) if k else 0
    return drv.frames[b].get(c, [])[before:res[k][b]["nframes"].get(c, 0)]


def check_model(model, drv, res, channels=None, b=0, calls=None, what=("audio", "status", "taps", "groups", "frames")):
    """every listed slot of batch b in every listed call of a serial run against the model"""
    channels = range(model.C[b]) if channels is None else channels
    for k in (range(len(res)) if calls is None else calls):
        r, n = res[k][b], model.script[k][0]
        for c in channels:
            m = model.at(k, c, b)
            if "audio" in what:
                assert _bits(r["audio"][c], m["audio"]), ("audio", k, n, c)
            if "status" in what and c in r["status"]:
                assert _status_equal(r["status"][c][0], m["status"]), ("status", k, n, c)
                assert r["status"][c][1] == k + 1, ("status call index", k, n, c)
            if "taps" in what and c in r["taps"]:
                for t in r["taps"][c]:
                    assert _bits(r["taps"][c][t], m["taps"][t]), (t, k, n, c)
            if "groups" in what and "groups" in r:
                got = [blk for ch, _, blk in r["groups"] if ch == c]
                assert got == m["groups"], ("groups", k, n, c, got, m["groups"])
            if "frames" in what and drv.callbacks:
                got = frames_of_call(drv, res, k, c, b)
                assert got == m["frames"], ("frames", k, n, c, got, m["frames"])


def check_names(model, drv, b=0, channels=None):
    """the PS name of every slot whose decoder began blank in it and has one at the end"""
    last = len(model.script) - 1
    for c in (range(model.C[b]) if channels is None else channels):
        name = model.at(last, c, b)["name"]
        if model.fresh[b][c] and name.strip():
            assert drv.names[b].get(c, [None])[-1] == name, ("name", c)


def taps_differ(model, res, k, c, b=0, names=("rds_lpf", "rds_mf")):
    """{tap: differs from the model's} of slot c in call k"""
    return {t: not _bits(res[k][b]["taps"][c][t], model.at(k, c, b)["taps"][t]) for t in names}


def check_same_runs(res, want, b=0, pairs=None, calls=None, what=("audio", "groups")):
    """channel g of `res` against channel w of `want` for (g, w) in pairs, call by call"""
    for k in (range(len(res)) if calls is None else calls):
        r, w = res[k][b], want[k][b]
        if pairs is None:
            assert r["audio"].shape == w["audio"].shape and r["audio"].tobytes() == w["audio"].tobytes(), ("audio", k)
            if "groups" in what and "groups" in r:
                assert r["groups"] == w["groups"], ("groups", k)
            continue
        for g_, w_ in pairs:
            assert _bits(r["audio"][g_], w["audio"][w_]), ("audio", k, g_, w_)
            if "groups" in what and "groups" in r:
                assert [x[1:] for x in r["groups"] if x[0] == g_] == [x[1:] for x in w["groups"] if x[0] == w_], \
                    ("groups", k, g_, w_)


# ---------------------------------------------------------------------------------------------------------------------
# the scripts (tests/test_edit_model_cpu.py shows on the oracle alone that they have bite)

F = N  # a full call
SHIFTS_B = [2, -4, 9, -9, 5, -2, 11, 6]  # batch B of two-batch scripts (tests/test_gpu_state.py); slot 4 tunes BSIDE
SHIFTS_2CAP = [LOUD, OTHER, MONO, -3, LOUD, 3, BSIDE, 10]  # over two captures: slots 4 and 6 wait for a switch


def rows_of(oracle, sizes, geom=GEOM):
    """the RDS rows of calls of these sizes (they depend on the sizes alone: one decoder on zeros)"""
    o = _oracle(oracle, 0, geom.fs, geom.d, geom.t, geom.order)
    out = []
    for n in sizes:
        o.process_stream(np.zeros(2 * n, np.float32))
        out.append(len(o.taps()["rds_mf"]))
    o.close()
    return out


def _steps(*items):
    """sizes and (size, edits) pairs as a script"""
    return [(x, []) if isinstance(x, (int, np.integer)) else (x[0], list(x[1])) for x in items]


SCRIPTS = {
    # 8 channels of SHIFTS0 on one shared capture: resets in front of a tiny call, behind a run of tiny calls, twice on
    # channel 0, around a whole-batch reset
    "resets": _steps(*[F] * 8, (88, [("reset", [0, 5])]), 88, 97, 150, 300, 170, 89, (100, [("reset", [1, 0])]), 3663,
                     330, 1001, F, (8191, [("reset", [2])]), F, F, (F, [("reset_all",)]), 171,
                     (12345, [("reset", [0, 3])]), 3662, 40000, 8192, *[F] * 9),
    # 8 channels, capture map over two rows (all on row 0), retuning enabled: retunes in front of and behind tiny
    # calls, to a capture, of a slot reset one call earlier
    "retunes": _steps(*[F] * 8, (88, [("retune", [3, 4], [LOUD, OTHER])]), 150, 300,
                      (F, [("retune", [5, 6], [BSIDE, LOUD], [1, 0])]), F, (97, [("reset", [2, 6])]),
                      (3663, [("retune", [2], [LOUD])]), 330, 100, (F, [("retune", [0, 1], [MONO, BSIDE], [0, 1])]),
                      *[F] * 8, (1001, [("retune", [7], [LOUD])]), 89, *[F] * 8),
    # SHIFTS_2CAP over two captures: switches in front of tiny calls, there and back
    "switches": _steps(*[F] * 8, (89, [("switch", [0, 4], [1, 1])]), 170, (300, [("switch", [0], [0])]), F,
                       (100, [("switch", [1, 2, 6], [1, 1, 1])]), (8191, [("switch", [1], [0])]), *[F] * 8,
                       (40000, [("switch", [3, 4], [1, 0])]), 3662, *[F] * 8),
    # batches A (SHIFTS0 on row 0) and B (SHIFTS_B on row 1): both saved behind an R = 1 call, destroyed and loaded;
    # A's channels 0, 1, 5 move into B's slots 6, 2, 3 behind tiny calls; saved again later
    "state": _steps(*[F] * 8, 88, (300, [("save_load",), (1, "save_load")]), 97, 3663,
                    (150, [("move", [0, 1, 5], [6, 2, 3]), (1, "switch", [6, 2, 3], [0, 0, 0])]), 170, 1001, *[F] * 8,
                    (89, [(1, "save_load")]), (8192, [("reset", [0]), (1, "reset", [6])]), *[F] * 8),
}
# 130 channels (three waves, the last partial) over two captures, two batches: every edit kind through one ragged
# script; the edited slots lie in every wave
SHIFTS_130 = [int(x) for x in np.resize(np.array([LOUD, OTHER, MONO, BSIDE], np.int32), 130)]
CMAP_130 = [0 if c < 70 else 1 for c in range(130)]
SCRIPTS["flight"] = _steps(
    *[F] * 7, (88, [("reset", [0, 64, 129]), (1, "reset", [5])]), 97,
    (300, [("retune", [1, 65, 128], [LOUD, LOUD, BSIDE])]),
    150, (F, [("switch", [4, 71], [1, 0])]), (170, [("save_load",)]), 3663,
    (1001, [("move", [0, 4, 129], [2, 66, 127]), (1, "switch", [2, 66, 127], [0, 1, 1])]), F,
    (F, [("reset_all",), (1, "reset_all")]), 171,
    (8191, [("retune", [6, 127], [LOUD, OTHER], [0, 0]), ("reset", [64])]),
    330, (12345, [(1, "save_load"), (1, "retune", [3], [LOUD])]), *[F] * 9)
# a shell of 16 384 channels (two sub-batches) on one shared capture, calls of at most 8192 samples; the edits are
# those of an 8-channel batch made on whole residue classes mod 8, so they lie on both sides of the border and in
# every wave
SCRIPTS["shell8"] = _steps(8192, 8192, (88, [("reset", [3, 0])]), 97, 300, 170,
                           (8191, [("retune", [5, 2], [LOUD, MONO])]),
                           150, (3663, [("reset", [5])]), 1001, (8192, [("reset_all",)]), 171,
                           (330, [("reset", [7]), ("retune", [1], [OTHER])]), 3662, 8192, 8192)


def widen(script, classes=8, channels=16384):
    """the script with every listed channel c replaced by its whole residue class c, c + classes, ..."""
    out = []
    for n, edits in script:
        wide = []
        for e in edits:
            if e[0] in ("reset", "retune", "switch"):
                cls = [list(range(c, channels, classes)) for c in e[1]]
                args = [[x for x, cl in zip(a, cls) for _ in cl] for a in e[2:]]
                wide.append((e[0], [c for cl in cls for c in cl], *args))
            else:
                wide.append(e)
        out.append((n, wide))
    return out


def long_streams(fmsig, geom, total):
    """two captures at another geometry, one stereo + RDS station each, three tuner steps below the centre (shift 3)"""
    f = -3.0 * geom.fs / geom.t
    sets = [[fmsig.default_params(geom.fs, f_offset=f, amp=0.3, noise_sigma=0.004, seed=41 + g, pi=0x7051 + g,
                                  ps="LONG%d" % g)] for g in range(2)]
    return Streams(fmsig, "long %g %d" % (geom.fs, geom.d), sets, total)


# shorter than the 1001-tap IF filter: 500, 700, 900, 333; a save / load behind the call of 700
SCRIPTS["long"] = _steps(F, (500, [("switch", [0], [1])]), 700, (900, [("save_load",), ("switch", [0, 1], [0, 1])]), F,
                         (333, [("switch", [1, 3], [0, 0])]), 1001, F)
SHIFTS_LONG, CMAP_LONG = [3, 3, 0, 3], [0, 0, 1, 1]

SETUPS = {"resets": (SHIFTS0, None, False), "retunes": (SHIFTS0, [0] * 8, True),
          "switches": (SHIFTS_2CAP, [0] * 8, True), "state": ([SHIFTS0, SHIFTS_B], [[0] * 8, [1] * 8], True),
          "flight": ([SHIFTS_130] * 2, [CMAP_130] * 2, True), "shell8": (SHIFTS0, None, False),
          "random": ([SHIFTS_2CAP, SHIFTS_B], [[0] * 8, [1] * 8], True)}
_built = {}


def build(oracle, fmsig, name, u8=False):
    """(script, streams, model, shifts, capture maps) of a named script ("random<seed>": random_script), built once"""
    if (name, u8) not in _built:
        script = random_script(oracle, int(name[6:])) if name.startswith("random") else SCRIPTS[name]
        shifts, cmaps, two = SETUPS["random" if name.startswith("random") else name]
        streams = main_streams(fmsig, total_samples(script), u8=u8, two=two)
        taps = RDS_TAPS + (("demod",) if name == "switches" else ())
        _built[(name, u8)] = (script, streams, Model(oracle, streams, script, shifts, cmaps, taps=taps), shifts, cmaps)
    return _built[(name, u8)]


RANDOM_SEEDS = (11, 12, 13)
KINDS = ("reset", "reset_all", "retune", "retune_to", "switch", "move", "save_load")


def random_script(oracle, seed, calls=24):
    """Two batches of 8 channels over two captures: 8 full calls, `calls` calls whose sizes are drawn from EDGES, from
    random values and (every third) full, with edits from the whole vocabulary in front of about every second, then 9
    full calls.  By construction: a per-channel reset only where both ring phases of its batch are non-zero; the
    first reset is followed by four calls of 88 .. 300 samples; every kind of edit occurs; a whole-batch reset
    reaches both batches (their clocks stay equal for the moves) and stands alone at its boundary; a save / load comes
    first at its boundary."""
    rng = np.random.default_rng(seed)
    sizes = [F] * 8
    for i in range(calls):
        u = rng.random()
        sizes.append(F if i % 3 == 2 else int(rng.choice(EDGES)) if u < 0.7 else int(rng.integers(88, 20000)))
    first_reset = 8 + int(rng.integers(1, 4))
    sizes[first_reset:first_reset + 5] = [int(rng.choice([88, 97, 300])), 88, int(rng.choice([89, 150, 170])), 100, 171]
    sizes += [F] * 9
    rows = rows_of(oracle, sizes)
    script = [(n, []) for n in sizes]
    since = 0  # the call of the last whole-batch reset
    must = list(KINDS)
    k = first_reset
    forced = ["reset"]
    while k < 8 + calls:
        ph = sum(rows[since:k])
        kind = forced.pop() if forced else must[int(rng.integers(len(must)))] if must and rng.random() < 0.6 \
            else KINDS[int(rng.integers(len(KINDS)))]
        b = int(rng.integers(2))
        ch = sorted(int(c) for c in rng.choice(8, size=int(rng.integers(1, 4)), replace=False))
        edits = script[k][1]
        if kind == "reset":
            if ph % T_LPF == 0 or ph % T_MF == 0:
                k += 1
                forced.append("reset")
                continue
            edits.append((b, "reset", ch))
        elif kind == "reset_all":
            edits[:] = [(0, "reset_all"), (1, "reset_all")]
            since = k
        elif kind in ("retune", "retune_to"):
            sh = [int(rng.choice([LOUD, OTHER, MONO, BSIDE, 0])) for _ in ch]
            edits.append((b, "retune", ch, sh) + (([int(rng.integers(2)) for _ in ch],) if kind == "retune_to" else ()))
        elif kind == "switch":
            edits.append((b, "switch", ch, [int(rng.integers(2)) for _ in ch]))
        elif kind == "move":
            dst = sorted(int(c) for c in rng.choice(8, size=len(ch), replace=False))
            edits.append(("move", ch, dst, b, 1 - b))
            edits.append((1 - b, "switch", dst, [int(rng.integers(2)) for _ in dst]))
        else:
            edits.insert(0, (b, "save_load"))
        if kind in must:
            must.remove(kind)
        k += 1 if kind == "reset_all" or rng.random() < 0.5 else 2
    assert not must, must
    return script
