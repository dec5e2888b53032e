"""Polyphase channeliser: a wideband capture's stations as channel IQ rows on the GPU (fmd_chan_*, include/fmd.h).

``Channeliser`` filters every capture once into its n_bins branch sums and rotates them into the wanted bins: one
complex64 row per station at sample_rate_in / decimation, exactly the rows a ``FMD_IN_CIQ_F32`` call of a ``Batch``
created at (sample_rate_in, decimation) takes in place of its IF stage (``make_call(ciq_in=rows)``), on the same
stream and without a copy.  ``plan_bins`` (host only) turns station offsets into the shifts.  Load through
``__graft_entry__.load_package()`` like the rest of the package.
"""
import ctypes as C

import numpy as np

from . import FMD_ERR_ARG_TEXT, FMD_IQ_F32, FmdChanParams, FmdError, _check, iq_format_of, lib

_TORCH_FORMATS = {"torch.complex64": (0, 1), "torch.float32": (0, 2), "torch.uint8": (1, 2), "torch.int8": (2, 2),
                  "torch.int16": (3, 2)}  # dtype -> (FMD_IQ_*, tensor elements per IQ sample)


class Channeliser:
    """n_captures captures x B rows (fmd_chan_create); shifts: [n_captures, B] (or flat, row r = g B + b) bins, any
    ints, taken mod n_bins: the row's centre is -shift * sample_rate_in / n_bins.  0 = the default of include/fmd.h:
    filter_order 8 * decimation, cutoff 0.6 / decimation, out_scale 1.0."""

    def __init__(self, sample_rate_in, n_bins, decimation, n_captures, shifts, filter_order=0, cutoff=0, out_scale=0,
                 device=0):
        sh = np.ascontiguousarray(shifts, dtype=np.int32).reshape(-1)
        G = int(n_captures)
        if G < 1 or sh.size == 0 or sh.size % G:
            raise FmdError(FMD_ERR_ARG_TEXT % "Channeliser: shifts must hold one entry per row for each of n_captures")
        self.params = FmdChanParams(float(sample_rate_in), int(n_bins), int(decimation), int(filter_order),
                                    float(cutoff), float(out_scale))
        h = C.c_void_p()
        _check(lib().fmd_chan_create(C.byref(self.params), G, sh.size // G, sh.ctypes.data, int(device), C.byref(h)))
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

    def out_stride(self, samples):
        """an even row stride that holds any call of `samples`"""
        return (self.max_out_samples(samples) + 1) & ~1

    def process(self, d_in, samples, out=None, stream=None, fmt=None, in_stride=None, out_stride=None):
        """One call on the device.  d_in: a torch tensor [n_captures, >= samples] (complex64) or [n_captures, >= 2
        samples] (float32 / uint8 / int8 / int16: I, Q, I, Q, ...), the format by its dtype, capture g in row g; or a
        device pointer with fmt (FMD_IQ_*) and in_stride (IQ samples).  out: a complex64 torch tensor [rows, even
        stride] (None: a new one of out_stride(samples)), or a device pointer with out_stride.  Returns (out, samples
        written to every row)."""
        import torch
        if isinstance(d_in, torch.Tensor):
            f, per = _TORCH_FORMATS.get(str(d_in.dtype), (None, None))
            if f is None:
                raise FmdError(FMD_ERR_ARG_TEXT % ("no IQ format for dtype %s" % d_in.dtype))
            t = d_in if d_in.dim() == 2 else d_in.reshape(1, -1)
            assert t.stride(1) == 1 and t.shape[0] == self.n_captures
            ptr, fmt = t.data_ptr(), f
            in_stride = t.stride(0) // per if self.n_captures > 1 else 0
        else:
            ptr = int(d_in)
            fmt = FMD_IQ_F32 if fmt is None else int(fmt)
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
        _check(lib().fmd_chan_process_device(self._h, ptr, fmt, int(in_stride), int(samples), optr, int(out_stride),
                                             C.byref(n), stream))
        return out, n.value

    def process_host(self, iq, out_stride=None):
        """iq: [n_captures, n] complex64, or [n_captures, 2 n] float32 / uint8 / int8 / int16 (I, Q, ...), in host
        memory; returns [rows, count] complex64 (out_stride: the stride of the buffer the rows are written into, any
        value >= the count -- odd ones too on this path).  Waits (fmd_chan_process_host)."""
        a, fmt, per = iq_format_of(np.asarray(iq).reshape(self.n_captures, -1))
        n = a.shape[1] // per
        stride = int(out_stride) if out_stride else max(self.max_out_samples(n), 1)
        out = np.zeros((self.rows, stride), np.complex64)
        m = C.c_uint()
        _check(lib().fmd_chan_process_host(self._h, a.ctypes.data, fmt, n, n, out.ctypes.data, stride, C.byref(m)))
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
