"""Band scan: which stations a batch's IQ captures hold (fmd_scan_*, include/fmd.h).

``Scan`` is the spectral scan on the GPU: an averaged power spectrum of every capture, read on the raster of the
decoder's tuner steps, with a list of candidate stations per capture.  ``scan_stations`` confirms the candidates
with a short decode on the existing batch decoder and reports stereo flag, pilot level, tuning offset, RDS PI and
PS name per station.  Load through ``__graft_entry__.load_package()`` like the rest of the package.
"""
import collections
import ctypes as C

import numpy as np

from . import (FMD_ERR_ARG_TEXT, FMD_IQ_F32, FMD_IQ_U8, SCAN_CANDIDATE_DTYPE, Batch, FmdError, FmdScanParams, _check,
               iq_format_of, lib, make_params)

_INTEGER_IQ = (np.dtype(np.uint8), np.dtype(np.int8), np.dtype(np.int16))


class Scan:
    """Spectral scan of n_captures captures (fmd_scan_create).  Defaults as in include/fmd.h: nfft 1024, a raster of
    table_size = 64 tuner steps, slots +-100 kHz wide, candidates 150 kHz apart and 10 dB over the floor, the floor
    at the 0.2 quantile of the bins."""

    def __init__(self, sample_rate_if, n_captures, table_size=64, nfft=1024, half_width_hz=100e3,
                 min_separation_hz=150e3, threshold_db=10.0, floor_quantile=0.2, device=0):
        # the C struct reads 0 as "default": an explicit 0 here is refused like any other value outside (0, 1)
        if not 0.0 < float(floor_quantile) < 1.0:
            raise FmdError(FMD_ERR_ARG_TEXT % "Scan: floor_quantile must lie strictly between 0 and 1")
        if not float(half_width_hz) > 0.0:
            raise FmdError(FMD_ERR_ARG_TEXT % "Scan: half_width_hz must be positive")
        self.params = FmdScanParams(float(sample_rate_if), int(table_size), int(nfft), float(half_width_hz),
                                    float(min_separation_hz), float(threshold_db), float(floor_quantile))
        h = C.c_void_p()
        _check(lib().fmd_scan_create(C.byref(self.params), int(n_captures), int(device), C.byref(h)))
        self._h = h
        self.n_captures = int(n_captures)
        self.nfft = int(nfft) or 1024
        self.sample_rate_if = float(sample_rate_if)
        first = C.c_int32()
        self.table_size = _check(lib().fmd_scan_slots(self._h, C.byref(first)))
        self.first_shift = first.value

    def close(self):
        if getattr(self, "_h", None):
            lib().fmd_scan_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def reset(self, stream=None):
        _check(lib().fmd_scan_reset(self._h, stream))

    def accumulate_device(self, ptr, stride, samples, stream=None, u8=False, fmt=None):
        """Capture g at ptr + 2*g*stride floats (bytes with u8=True), `samples` IQ samples each; fmt (FMD_IQ_*): the
        captures' format, stride in IQ samples (fmd_scan_accumulate_device_fmt)."""
        if fmt is not None:
            _check(lib().fmd_scan_accumulate_device_fmt(self._h, ptr, int(fmt), int(stride), int(samples), stream))
            return
        fn = lib().fmd_scan_accumulate_device_u8 if u8 else lib().fmd_scan_accumulate_device
        _check(fn(self._h, ptr, int(stride), int(samples), stream))

    def accumulate_host(self, iq):
        """iq: [G, n] complex64 (or float32 [G, 2n]); [n] for a single capture.  uint8 / int8 / int16 arrays [G, 2n]
        are integer IQ of that format (fmd_scan_accumulate_host_fmt), converted on the device like the decoder's."""
        iq = np.ascontiguousarray(iq)
        if iq.dtype in _INTEGER_IQ:
            iq, fmt, _ = iq_format_of(iq.reshape(self.n_captures, -1))
            n = iq.shape[1] // 2
            _check(lib().fmd_scan_accumulate_host_fmt(self._h, iq.ctypes.data, fmt, n, n))
            return
        if iq.dtype != np.complex64:
            iq = np.ascontiguousarray(iq, dtype=np.float32).view(np.complex64)
        iq = iq.reshape(self.n_captures, -1)
        n = iq.shape[1]
        _check(lib().fmd_scan_accumulate_host(self._h, iq.ctypes.data, n, n))

    def accumulate_host_u8(self, buf):
        """buf: [G, 2n] RTL-SDR byte pairs; converted on the device exactly like the decoder converts them."""
        import torch
        buf = np.ascontiguousarray(buf, dtype=np.uint8).reshape(self.n_captures, -1)
        n = buf.shape[1] // 2
        d = torch.from_numpy(buf).cuda()
        stream = torch.cuda.current_stream().cuda_stream
        self.accumulate_device(d.data_ptr(), n, n, stream=stream, u8=True)
        torch.cuda.current_stream().synchronize()

    def shifts(self):
        return np.arange(self.table_size, dtype=np.int32) + self.first_shift

    def finish_device(self, psd=None, slot_db=None, floor_db=None, cand=None, max_cand=0, counts=None, stream=None):
        """fmd_scan_finish_device: device pointers (None: not written) of psd [G, N], slot_db [G, T], floor_db [G]
        (float32), cand [G, max_cand] (SCAN_CANDIDATE_DTYPE) and counts [G] (uint32), written asynchronously on
        stream.  Nothing is reset."""
        _check(lib().fmd_scan_finish_device(self._h, psd, slot_db, floor_db, cand, int(max_cand), counts, stream))

    def result(self, max_cand=None):
        """The scan so far (nothing is reset): psd [G, N] (bin i at (i - N/2) fs / N), freqs [N], shifts [T],
        slot_hz [T], slot_db [G, T] (-inf: ineligible), floor_db [G], candidates (per capture a list of dicts with
        shift, offset_hz, power_db, snr_db, by increasing frequency)."""
        G, N, T = self.n_captures, self.nfft, self.table_size
        cap = T if max_cand is None else int(max_cand)
        psd = np.zeros((G, N), np.float32)
        slot_db = np.zeros((G, T), np.float32)
        floor_db = np.zeros(G, np.float32)
        cand = np.zeros((G, max(cap, 1)), SCAN_CANDIDATE_DTYPE)
        counts = np.zeros(G, np.uint32)
        _check(lib().fmd_scan_finish_host(self._h, psd.ctypes.data, slot_db.ctypes.data, floor_db.ctypes.data,
                                          cand.ctypes.data, cap, counts.ctypes.data))
        fs = self.sample_rate_if
        shifts = self.shifts()
        cands = [[{k: (int(c[k]) if k == "shift" else float(c[k])) for k in SCAN_CANDIDATE_DTYPE.names}
                  for c in cand[g, :min(int(counts[g]), cap)]] for g in range(G)]
        return {"psd": psd, "freqs": (np.arange(N) - N / 2) * fs / N, "shifts": shifts,
                "slot_hz": -shifts.astype(np.float64) * fs / T, "slot_db": slot_db, "floor_db": floor_db,
                "candidates": cands, "counts": counts}


def scan_stations(source, n_captures, sample_rate_if, table_size=24, scan_calls=4, confirm_calls=48, center_hz=None,
                  u8=False, **scan_kw):
    """Find the stations of n_captures captures.  source(call) -> [G, n] complex64 captures (u8=True: [G, 2n]
    RTL-SDR bytes; int8 / int16 arrays [G, 2n]: signed integer IQ, taken by their dtype) of one call; calls 0 .. scan_calls-1 go through the spectral scan, the next confirm_calls through
    one decoder batch with a channel per candidate (the tuner dialog's 1.25 s dwell at 2.4 MS/s and n = 65 536).
    Returns per capture a list of stations by increasing frequency: shift, offset_hz (or freq_hz = center_hz +
    offset when center_hz is given), power_db, snr_db, stereo, pilot_level, tuning_offset, pi (the most frequent
    block A among the channel's groups, or None), ps (the PS name, or None).  Nothing is filtered out.
    scan_kw: Scan's keywords, and downsample (the decoder's; default: the one nearest fs / 218 kHz)."""
    fs = float(sample_rate_if)
    downsample = int(scan_kw.pop("downsample", max(1, int(round(fs / 218.18e3)))))
    G = int(n_captures)
    scan = Scan(fs, G, table_size=table_size, **scan_kw)
    try:
        for call in range(scan_calls):
            x = source(call)
            if u8:
                scan.accumulate_host_u8(x)
            else:
                scan.accumulate_host(x)
        cands = scan.result()["candidates"]
    finally:
        scan.close()
    k = max((len(c) for c in cands), default=0)
    out = [[] for _ in range(G)]
    if k == 0:
        return out
    # one channel per candidate, k per capture; captures with fewer candidates repeat their first (or shift 0)
    shifts = np.zeros((G, k), np.int32)
    for g, cs in enumerate(cands):
        for j in range(k):
            shifts[g, j] = cs[j]["shift"] if j < len(cs) else (cs[0]["shift"] if cs else 0)
    b = Batch(make_params(fs, 0.0, 48000.0, 15000.0, downsample, table_size=table_size), G * k,
              tuning_shifts=shifts.reshape(-1))
    try:
        import torch
        b.set_channels_per_capture(k)
        blocks = collections.defaultdict(collections.Counter)
        stream = torch.cuda.current_stream()
        for call in range(scan_calls, scan_calls + confirm_calls):
            # device calls: the groups stay queued for collect_rds (a host call would drain them itself)
            x = np.ascontiguousarray(source(call))
            fmt = FMD_IQ_U8 if u8 else FMD_IQ_F32
            if not u8 and x.dtype in _INTEGER_IQ[1:]:
                x, fmt, _ = iq_format_of(x)
            elif not u8 and x.dtype == np.complex64:
                x = x.view(np.float32)
            d = torch.from_numpy(x.reshape(G, -1)).cuda()
            n = d.shape[1] // 2
            a_stride = b.max_audio_floats(n)
            audio = torch.empty((G * k, a_stride), dtype=torch.float32, device="cuda")
            b.process_device(d.data_ptr(), n, n, audio.data_ptr(), a_stride, stream=stream.cuda_stream, fmt=fmt)
            groups = b.collect_rds_array(run_group_decoder=True, stream=stream.cuda_stream)
            for ch, blk in zip(groups["channel"], groups["blocks"]):
                blocks[int(ch)][int(blk[0])] += 1
        for g, cs in enumerate(cands):
            for j, c in enumerate(cs):
                ch = g * k + j
                st = b.status(ch)
                cnt = blocks.get(ch)
                station = dict(c)
                if center_hz is not None:
                    station["freq_hz"] = float(center_hz) + station.pop("offset_hz")
                station.update(stereo=bool(st.stereo_detected), pilot_level=float(st.pilot_level),
                               tuning_offset=float(st.tuning_offset),
                               pi=cnt.most_common(1)[0][0] if cnt else None,
                               ps=b.sink.names.get(ch))
                out[g].append(station)
    finally:
        b.close()
    return out
