"""Polyphase channeliser: a wideband capture's stations as channel IQ rows on the GPU (fmd_chan_*, include/fmd.h).

``Channeliser`` filters every capture once into its n_bins branch sums and rotates them into the wanted bins: one
complex64 row per station at sample_rate_in / decimation, exactly the rows a ``FMD_IN_CIQ_F32`` call of a ``Batch``
created at (sample_rate_in, decimation) takes in place of its IF stage (``make_call(ciq_in=rows)``), on the same
stream and without a copy.  ``rows=np.int16`` on a call gives the rows as int16 (re, im) pairs instead, what a
``FMD_IN_CIQ_S16`` call takes.  ``Channeliser(..., real=True)`` takes real-sampled captures (one element per sample,
n_bins up to 512).  ``plan_bins`` (host only) turns station offsets into the shifts, ``plan_bins_real`` the RF
frequencies of stations in a real-sampled capture.  Load through ``__graft_entry__.load_package()`` like the rest of
the package.
"""
import ctypes as C

import numpy as np

from . import (FMD_CIQ_F32, FMD_CIQ_S16, FMD_ERR_ARG_TEXT, FMD_IQ_F32, FMD_REAL_F32, FMD_REAL_S8, FMD_REAL_S16,
               FmdChanParams, FmdError, _check, iq_format_of, lib)

_TORCH_FORMATS = {"torch.complex64": (0, 1), "torch.float32": (0, 2), "torch.uint8": (1, 2), "torch.int8": (2, 2),
                  "torch.int16": (3, 2)}  # dtype -> (FMD_IQ_*, tensor elements per IQ sample)
_TORCH_REAL_FORMATS = {"torch.float32": FMD_REAL_F32, "torch.int8": FMD_REAL_S8, "torch.int16": FMD_REAL_S16}
_NUMPY_REAL_FORMATS = {np.dtype(np.float32): FMD_REAL_F32, np.dtype(np.int8): FMD_REAL_S8,
                       np.dtype(np.int16): FMD_REAL_S16}


def rows_format_of(rows):
    """FMD_CIQ_* of a `rows=` argument: None or np.complex64 (the default), np.int16, or the constant itself."""
    if rows is None:
        return FMD_CIQ_F32
    if isinstance(rows, (int, np.integer)) and not isinstance(rows, bool):
        if int(rows) in (FMD_CIQ_F32, FMD_CIQ_S16):
            return int(rows)
    else:
        try:
            dt = np.dtype(rows)
        except TypeError:
            dt = None
        if dt == np.dtype(np.complex64):
            return FMD_CIQ_F32
        if dt == np.dtype(np.int16):
            return FMD_CIQ_S16
    raise FmdError(FMD_ERR_ARG_TEXT % ("no row format for %r (complex64, int16, FMD_CIQ_F32, FMD_CIQ_S16)" % (rows,)))


class Channeliser:
    """n_captures captures x B rows (fmd_chan_create); shifts: [n_captures, B] (or flat, row r = g B + b) bins, any
    ints, taken mod n_bins: the row's centre is -shift * sample_rate_in / n_bins.  0 = the default of include/fmd.h:
    filter_order 8 * decimation, cutoff 0.6 / decimation, out_scale 1.0.  real=True: real-sampled captures
    (fmd_chan_create_real), sample_rate_in the real sample rate, n_bins up to 512; for life."""

    def __init__(self, sample_rate_in, n_bins, decimation, n_captures, shifts, filter_order=0, cutoff=0, out_scale=0,
                 device=0, real=False):
        sh = np.ascontiguousarray(shifts, dtype=np.int32).reshape(-1)
        G = int(n_captures)
        if G < 1 or sh.size == 0 or sh.size % G:
            raise FmdError(FMD_ERR_ARG_TEXT % "Channeliser: shifts must hold one entry per row for each of n_captures")
        self.params = FmdChanParams(float(sample_rate_in), int(n_bins), int(decimation), int(filter_order),
                                    float(cutoff), float(out_scale))
        self.real = bool(real)
        h = C.c_void_p()
        create = lib().fmd_chan_create_real if self.real else lib().fmd_chan_create
        _check(create(C.byref(self.params), G, sh.size // G, sh.ctypes.data, int(device), C.byref(h)))
        self._h = h
        self.n_captures, self.n_rows_per_capture = G, sh.size // G
        self.n_bins, self.decimation = int(n_bins), int(decimation)
        self.rows = _check(lib().fmd_chan_rows(self._h))
        self.out_rate = float(lib().fmd_chan_out_rate(self._h))
        self.tile_samples = int(lib().fmd_chan_tile_samples(self._h))

    def close(self):
        if getattr(self, "_h", None):
            lib().fmd_chan_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def reset(self, stream=None):
        """zero history, q = 0 (fmd_chan_reset), asynchronously on stream"""
        _check(lib().fmd_chan_reset(self._h, stream))

    def set_shifts(self, shifts):
        """New shifts for all rows from the next call submitted (fmd_chan_set_shifts): every row then has the bits of
        a channeliser that had them from the start.  Does not wait for the device."""
        sh = np.ascontiguousarray(shifts, dtype=np.int32).reshape(-1)
        _check(lib().fmd_chan_set_shifts(self._h, sh.ctypes.data, sh.size))

    def taps(self):
        """the K taps in use, c[1 .. K]"""
        k = _check(lib().fmd_chan_get_taps(self._h, None, 0))
        out = np.zeros(k, np.float32)
        _check(lib().fmd_chan_get_taps(self._h, out.ctypes.data, k))
        return out

    def max_out_samples(self, samples):
        return int(lib().fmd_chan_max_out_samples(self._h, int(samples)))

    def out_stride(self, samples, rows=None):
        """a row stride that holds any call of `samples`: even, for rows=np.int16 a multiple of 4"""
        al = 3 if rows_format_of(rows) == FMD_CIQ_S16 else 1
        return (self.max_out_samples(samples) + al) & ~al

    def process(self, d_in, samples, out=None, stream=None, fmt=None, in_stride=None, out_stride=None, rows=None):
        """One call on the device.  d_in: a torch tensor [n_captures, >= samples] (complex64) or [n_captures, >= 2
        samples] (float32 / uint8 / int8 / int16: I, Q, I, Q, ...), the format by its dtype, capture g in row g; a real
        channeliser: [n_captures, >= samples] float32 / int8 / int16, one element per sample; or a device pointer with
        fmt (FMD_IQ_* / FMD_REAL_*) and in_stride (samples).  rows: np.complex64 (default) or np.int16.  out: a
        complex64 torch tensor [rows, even stride], for rows=np.int16 an int16 one [rows, stride, 2] with the stride a
        multiple of 4 (None: a new one of out_stride(samples, rows)), or a device pointer with out_stride.  Returns
        (out, samples written to every row)."""
        import torch
        ofmt = rows_format_of(rows)
        if isinstance(d_in, torch.Tensor):
            if self.real:
                f, per = _TORCH_REAL_FORMATS.get(str(d_in.dtype)), 1
            else:
                f, per = _TORCH_FORMATS.get(str(d_in.dtype), (None, None))
            if f is None:
                raise FmdError(FMD_ERR_ARG_TEXT % ("no %s format for dtype %s" % ("real-sample" if self.real else "IQ",
                                                                                  d_in.dtype)))
            t = d_in if d_in.dim() == 2 else d_in.reshape(1, -1)
            assert t.stride(1) == 1 and t.shape[0] == self.n_captures
            ptr, fmt = t.data_ptr(), f
            in_stride = t.stride(0) // per if self.n_captures > 1 else 0
        else:
            ptr = int(d_in)
            fmt = (FMD_REAL_F32 if self.real else FMD_IQ_F32) if fmt is None else int(fmt)
            in_stride = int(in_stride or 0)
        if out is None:
            stride = self.out_stride(samples, rows)
            if ofmt == FMD_CIQ_S16:
                out = torch.empty((self.rows, stride, 2), dtype=torch.int16, device="cuda")
            else:
                out = torch.empty((self.rows, stride), dtype=torch.complex64, device="cuda")
        if isinstance(out, torch.Tensor):
            if ofmt == FMD_CIQ_S16:
                assert out.dtype == torch.int16 and out.shape[-1] == 2 and out.stride(-1) == 1 and out.stride(-2) == 2
                optr, out_stride = out.data_ptr(), (out.stride(0) // 2 if out.dim() == 3 else out.numel() // 2)
            else:
                assert out.dtype == torch.complex64 and out.stride(-1) == 1
                optr, out_stride = out.data_ptr(), (out.stride(0) if out.dim() == 2 else out.numel())
        else:
            optr, out_stride = int(out), int(out_stride)
        if stream is None:
            stream = torch.cuda.current_stream().cuda_stream
        n = C.c_uint()
        _check(lib().fmd_chan_process_device_fmt(self._h, ptr, fmt, int(in_stride), int(samples), optr, ofmt,
                                                 int(out_stride), C.byref(n), stream))
        return out, n.value

    def process_host(self, iq, out_stride=None, rows=None):
        """iq: [n_captures, n] complex64, or [n_captures, 2 n] float32 / uint8 / int8 / int16 (I, Q, ...), in host
        memory; a real channeliser: [n_captures, n] float32 / int8 / int16.  Returns [rows, count] complex64, for
        rows=np.int16 [rows, count, 2] int16 (out_stride: the stride of the buffer the rows are written into, any
        value >= the count -- odd ones too on this path).  Waits (fmd_chan_process_host_fmt)."""
        ofmt = rows_format_of(rows)
        if self.real:
            a = np.ascontiguousarray(np.asarray(iq).reshape(self.n_captures, -1))
            fmt, per = _NUMPY_REAL_FORMATS.get(a.dtype), 1
            if fmt is None:
                raise FmdError(FMD_ERR_ARG_TEXT % ("no real-sample format for dtype %s (float32, int8, int16)"
                                                   % a.dtype))
        else:
            a, fmt, per = iq_format_of(np.asarray(iq).reshape(self.n_captures, -1))
        n = a.shape[1] // per
        stride = int(out_stride) if out_stride else max(self.max_out_samples(n), 1)
        if ofmt == FMD_CIQ_S16:
            out = np.zeros((self.rows, stride, 2), np.int16)
        else:
            out = np.zeros((self.rows, stride), np.complex64)
        m = C.c_uint()
        _check(lib().fmd_chan_process_host_fmt(self._h, a.ctypes.data, fmt, n, n, out.ctypes.data, ofmt, stride,
                                               C.byref(m)))
        return out[:, :m.value]


def plan_bins(sample_rate_in, n_bins, station_offsets_hz, tolerance_hz=1e3):
    """The shifts of stations at station_offsets_hz (Hz from the capture's centre), for Channeliser.  Host only.

    Bin k of n_bins lies at k * sample_rate_in / n_bins, and a row with shift s is centred on -s * sample_rate_in /
    n_bins, so the station at offset f gets shift -round(f n_bins / sample_rate_in), in [-n_bins / 2, n_bins / 2].
    A station more than tolerance_hz (1 kHz) off the raster, or beyond +-sample_rate_in / 2, is refused with a
    ValueError that names it: the channeliser has no fine tuner behind the bank."""
    fs, N = float(sample_rate_in), int(n_bins)
    if not fs > 0 or N < 2:
        raise ValueError("plan_bins: sample_rate_in must be positive and n_bins at least 2")
    step = fs / N
    shifts = []
    for f in np.asarray(station_offsets_hz, dtype=np.float64).reshape(-1):
        k = int(np.floor(f / step + 0.5))
        if abs(f) > fs / 2:
            raise ValueError("plan_bins: the station at %g Hz lies outside the capture (+-%g Hz)" % (f, fs / 2))
        if abs(f - k * step) > float(tolerance_hz):
            raise ValueError("plan_bins: the station at %g Hz is %g Hz off the raster of %g Hz (n_bins %d at %g S/s), "
                             "more than %g Hz" % (f, f - k * step, step, N, fs, float(tolerance_hz)))
        shifts.append(-k)
    return shifts


def plan_bins_real(sample_rate_in, n_bins, station_rf_hz, tolerance_hz=1e3, guard_hz=200e3):
    """plan_bins for a real-sampled capture, from the stations' RF frequencies, for Channeliser(..., real=True).  Host
    only.

    Sampling a real signal at fs folds every Nyquist zone onto [-fs/2, fs/2): the station at RF f appears, un-inverted,
    at f - round(f / fs) * fs -- a positive offset out of an odd zone, a negative one out of an even zone (split.py's
    plan_bands_real).  A station within guard_hz of 0 or of +-fs/2 lies on its own mirror and cannot be received:
    ValueError.  The offsets then go through plan_bins' raster rule."""
    fs = float(sample_rate_in)
    if not fs > 0 or not guard_hz >= 0:
        raise ValueError("plan_bins_real: sample_rate_in must be positive and guard_hz not negative")
    f = np.asarray(station_rf_hz, dtype=np.float64).reshape(-1)
    off = f - np.floor(f / fs + 0.5) * fs          # [-fs/2, fs/2)
    for rf, o in zip(f, off):
        if abs(o) < guard_hz or fs / 2 - abs(o) < guard_hz:
            raise ValueError("plan_bins_real: the station at %g Hz folds to %g Hz, within %g Hz of 0 or fs/2 = %g Hz: "
                             "it lies on its own mirror" % (rf, o, guard_hz, fs / 2))
    return plan_bins(fs, n_bins, off, tolerance_hz)
