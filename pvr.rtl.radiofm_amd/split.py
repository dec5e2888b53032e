"""Band splitter: wideband captures into decoder-rate bands on the GPU (fmd_split_*, include/fmd.h).

``Splitter`` mixes and decimates every capture once into a few overlapping bands at sample_rate_in / decimation --
ordinary complex64 captures for a ``Batch`` created at that rate, whose channels read their band through
``Batch.set_capture_map``.  ``plan_bands`` (host only) places the bands over a list of station offsets and says which
band and which offset inside it every station gets.  ``Splitter(..., real=True)`` takes real-sampled captures (an
Airspy in raw mode, a direct-sampling ADC: FMD_REAL_*), and ``plan_bands_real`` plans their bands from the stations'
RF frequencies, whatever the Nyquist zone.  Load through ``__graft_entry__.load_package()`` like the rest of
the package.
"""
import ctypes as C
import math

import numpy as np

from . import (FMD_ERR_ARG_TEXT, FMD_IQ_F32, FMD_REAL_F32, FMD_REAL_S8, FMD_REAL_S16, FmdError, FmdSplitParams, _check,
               iq_format_of, lib)

_TORCH_FORMATS = {"torch.complex64": (0, 1), "torch.float32": (0, 2), "torch.uint8": (1, 2), "torch.int8": (2, 2),
                  "torch.int16": (3, 2)}  # dtype -> (FMD_IQ_*, tensor elements per IQ sample)
# a real splitter's input, one element per sample: the dtype alone is ambiguous with interleaved IQ, the kind decides
_TORCH_REAL_FORMATS = {"torch.float32": FMD_REAL_F32, "torch.int8": FMD_REAL_S8, "torch.int16": FMD_REAL_S16}
_NUMPY_REAL_FORMATS = {np.dtype(np.float32): FMD_REAL_F32, np.dtype(np.int8): FMD_REAL_S8,
                       np.dtype(np.int16): FMD_REAL_S16}


class Splitter:
    """n_captures captures x B bands (fmd_split_create); shifts: [n_captures, B] (or flat, row r = g B + b) tuner
    shifts, the band's centre is -shift * sample_rate_in / table_size.  0 = the default of include/fmd.h: filter_order
    8 * decimation, cutoff 0.6 / decimation, table_size 64, out_scale 0.5.  real=True: a splitter of real-sampled
    captures (fmd_split_create_real), sample_rate_in the real sample rate; it takes float32 / int8 / int16 input with
    one element per sample and nothing else, a complex splitter only IQ."""

    def __init__(self, sample_rate_in, decimation, n_captures, shifts, filter_order=0, cutoff=0, table_size=0,
                 out_scale=0, device=0, real=False):
        sh = np.ascontiguousarray(shifts, dtype=np.int32).reshape(-1)
        G = int(n_captures)
        if G < 1 or sh.size == 0 or sh.size % G:
            raise FmdError(FMD_ERR_ARG_TEXT % "Splitter: shifts must hold n_bands entries for each of n_captures")
        self.params = FmdSplitParams(float(sample_rate_in), int(decimation), int(filter_order), float(cutoff),
                                     int(table_size), float(out_scale))
        h = C.c_void_p()
        self.real = bool(real)
        create = lib().fmd_split_create_real if self.real else lib().fmd_split_create
        _check(create(C.byref(self.params), G, sh.size // G, sh.ctypes.data, int(device), C.byref(h)))
        self._h = h
        self.n_captures, self.n_bands = G, sh.size // G
        self.decimation = int(decimation)
        self.rows = _check(lib().fmd_split_rows(self._h))
        self.out_rate = float(lib().fmd_split_out_rate(self._h))
        self.tile_samples = int(lib().fmd_split_tile_samples(self._h))

    def close(self):
        if getattr(self, "_h", None):
            lib().fmd_split_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def reset(self, stream=None):
        """zero history, q = 0 (fmd_split_reset), asynchronously on stream"""
        _check(lib().fmd_split_reset(self._h, stream))

    def set_shifts(self, shifts):
        """New shifts for all rows from the next call submitted (fmd_split_set_shifts): every row then has the bits
        of a splitter that had them from the start.  Does not wait for the device."""
        sh = np.ascontiguousarray(shifts, dtype=np.int32).reshape(-1)
        _check(lib().fmd_split_set_shifts(self._h, sh.ctypes.data, sh.size))

    def taps(self):
        """the K taps in use, c[1 .. K]"""
        k = _check(lib().fmd_split_get_taps(self._h, None, 0))
        out = np.zeros(k, np.float32)
        _check(lib().fmd_split_get_taps(self._h, out.ctypes.data, k))
        return out

    def debug_table_versions(self):
        """Testing aid: how many staging versions of the tuner tables exist (fmd_split_debug_table_versions)."""
        return _check(lib().fmd_split_debug_table_versions(self._h))

    def max_out_samples(self, samples):
        return int(lib().fmd_split_max_out_samples(self._h, int(samples)))

    def out_stride(self, samples):
        """an even row stride that holds any call of `samples`"""
        return (self.max_out_samples(samples) + 1) & ~1

    def process(self, d_in, samples, out=None, stream=None, fmt=None, in_stride=None, out_stride=None):
        """One call on the device.  d_in: a torch tensor [n_captures, >= samples] (complex64) or [n_captures, >= 2
        samples] (float32 / uint8 / int8 / int16: I, Q, I, Q, ...), the format by its dtype like the batch's input,
        capture g in row g; or a device pointer with fmt (FMD_IQ_*) and in_stride (IQ samples).  A real splitter:
        [n_captures, >= samples] float32 / int8 / int16, one element per sample, rows a multiple of four samples apart
        (or a pointer with fmt FMD_REAL_* and in_stride in real samples).  out: a complex64
        torch tensor [rows, even stride] (None: a new one of out_stride(samples)), or a device pointer with
        out_stride.  Returns (out, samples written to every row)."""
        import torch
        if isinstance(d_in, torch.Tensor):
            if self.real:
                f, per = _TORCH_REAL_FORMATS.get(str(d_in.dtype)), 1
            else:
                f, per = _TORCH_FORMATS.get(str(d_in.dtype), (None, None))
            if f is None:
                raise FmdError(FMD_ERR_ARG_TEXT % ("no %s format for dtype %s" % ("real-sample (float32, int8, int16)"
                                                                                  if self.real else "IQ", d_in.dtype)))
            t = d_in if d_in.dim() == 2 else d_in.reshape(1, -1)
            assert t.stride(1) == 1 and t.shape[0] == self.n_captures
            ptr, fmt = t.data_ptr(), f
            in_stride = t.stride(0) // per if self.n_captures > 1 else 0
        else:
            ptr = int(d_in)
            fmt = (FMD_REAL_F32 if self.real else FMD_IQ_F32) if fmt is None else int(fmt)
            in_stride = int(in_stride or 0)
        if out is None:
            out = torch.empty((self.rows, self.out_stride(samples)), dtype=torch.complex64, device="cuda")
        if isinstance(out, torch.Tensor):
            assert out.dtype == torch.complex64 and out.stride(-1) == 1
            optr, out_stride = out.data_ptr(), (out.stride(0) if out.dim() == 2 else out.numel())
        else:
            optr, out_stride = int(out), int(out_stride)
        if stream is None:
            stream = torch.cuda.current_stream().cuda_stream
        n = C.c_uint()
        _check(lib().fmd_split_process_device(self._h, ptr, fmt, int(in_stride), int(samples), optr, int(out_stride),
                                              C.byref(n), stream))
        return out, n.value

    def process_host(self, iq, out_stride=None):
        """iq: [n_captures, n] complex64, or [n_captures, 2 n] float32 / uint8 / int8 / int16 (I, Q, ...), in host
        memory; returns [rows, count] complex64 (out_stride: the stride of the buffer the rows are written into, any
        value >= the count -- odd ones too on this path).  A real splitter: [n_captures, n] float32 / int8 / int16.
        Waits (fmd_split_process_host)."""
        if self.real:
            a, per = np.ascontiguousarray(np.asarray(iq).reshape(self.n_captures, -1)), 1
            fmt = _NUMPY_REAL_FORMATS.get(a.dtype)
            if fmt is None:
                raise FmdError(FMD_ERR_ARG_TEXT % ("no real-sample format for dtype %s (float32, int8, int16)"
                                                   % a.dtype))
        else:
            a, fmt, per = iq_format_of(np.asarray(iq).reshape(self.n_captures, -1))
        n = a.shape[1] // per
        stride = int(out_stride) if out_stride else max(self.max_out_samples(n), 1)
        out = np.zeros((self.rows, stride), np.complex64)
        m = C.c_uint()
        _check(lib().fmd_split_process_host(self._h, a.ctypes.data, fmt, n, n, out.ctypes.data, stride, C.byref(m)))
        return out[:, :m.value]


def plan_bands(sample_rate_in, decimation, table_size, station_offsets_hz, usable_half_width_hz):
    """Cover station offsets (Hz from the wideband capture's centre) with splitter bands.  Host only.

    A band's centre lies on the tuner raster, -shift * sample_rate_in / table_size.  Greedy from the lowest station:
    the band is put as high as the raster allows with that station still inside usable_half_width_hz, and takes
    every station within usable_half_width_hz of its centre.  Returns (shifts, where): the bands' tuner shifts (ints,
    for Splitter) and per station, in the order given, (band index, offset inside the band in Hz) -- the offset is
    what fmd_batch_create's tuning_offset / tuning_shifts take at the band's rate, the band index what
    set_capture_map takes (plus g * n_bands for capture g).

    The usable half width for a given cutoff: the band's filter passes up to cutoff * sample_rate_in and what lies
    beyond sample_rate_in / decimation - cutoff * sample_rate_in folds back onto it, so a band at fs_out =
    sample_rate_in / decimation is alias-free within (1 - cutoff * decimation) * fs_out of its centre; a station
    needs its own 100 kHz of that, so usable_half_width_hz = (1 - cutoff * decimation) * fs_out - 100e3 (860 kHz at
    fs_out = 2.4 MS/s with the default cutoff 0.6 / decimation).  Raises ValueError when the raster is too coarse to
    put a band within the usable width of a station."""
    fs, T = float(sample_rate_in), int(table_size)
    if not fs > 0 or T < 1 or int(decimation) < 2 or not usable_half_width_hz > 0:
        raise ValueError("plan_bands: sample_rate_in, table_size, decimation and usable_half_width_hz must be positive")
    step = fs / T
    usable = float(usable_half_width_hz)
    f = np.asarray(station_offsets_hz, dtype=np.float64).reshape(-1)
    order = np.argsort(f, kind="stable")
    where = [None] * f.size
    shifts = []
    i = 0
    while i < order.size:
        f0 = f[order[i]]
        k = math.floor((f0 + usable) / step + 1e-9)      # the highest raster point with f0 still inside
        k = max(-(T // 2), min(T // 2, k))
        centre = k * step
        if abs(f0 - centre) > usable + 1e-6:
            raise ValueError("plan_bands: no raster point (step %g Hz) within %g Hz of the station at %g Hz"
                             % (step, usable, f0))
        band = len(shifts)
        shifts.append(int(-k))
        while i < order.size and f[order[i]] - centre <= usable + 1e-6:
            where[order[i]] = (band, float(f[order[i]] - centre))
            i += 1
    return shifts, where


def plan_bands_real(sample_rate_in, decimation, table_size, station_rf_hz, usable_half_width_hz, guard_hz=200e3):
    """plan_bands for a real-sampled capture, from the stations' RF frequencies.  Host only.

    Sampling a real signal at fs folds every Nyquist zone onto [-fs/2, fs/2): the station at RF f appears, un-inverted,
    at f - round(f / fs) * fs -- a positive offset out of an odd zone (1: 0 .. fs/2, 3: fs .. 3 fs/2, ...), a
    negative one out of an even zone (2: fs/2 .. fs, ...) -- and inverted at minus that.  A station within guard_hz
    of 0 or of +-fs/2 lies on its own mirror and cannot be received: ValueError.  The offsets go to plan_bands;
    returns its (shifts, where), for Splitter(..., real=True)."""
    fs = float(sample_rate_in)
    if not fs > 0 or not guard_hz >= 0:
        raise ValueError("plan_bands_real: sample_rate_in must be positive and guard_hz not negative")
    f = np.asarray(station_rf_hz, dtype=np.float64).reshape(-1)
    off = f - np.floor(f / fs + 0.5) * fs          # [-fs/2, fs/2)
    for rf, o in zip(f, off):
        if abs(o) < guard_hz or fs / 2 - abs(o) < guard_hz:
            raise ValueError("plan_bands_real: the station at %g Hz folds to %g Hz, within %g Hz of 0 or fs/2 = %g Hz: "
                             "it lies on its own mirror" % (rf, o, guard_hz, fs / 2))
    return plan_bands(fs, decimation, table_size, off, usable_half_width_hz)
