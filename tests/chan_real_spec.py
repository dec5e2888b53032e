"""The real-sampled channeliser and the int16 rows (include/fmd.h, fmd_chan_create_real, the _fmt entry points) in
numpy: what tests/test_chan_real_spec_cpu.py and tests/test_gpu_chan_real.py hold the device against.

  x[q] = (convert(v[q]), +0.0f), then the channeliser's definition as it stands: `truth` and `reference_rows` are
  chan_spec's on those pairs.
  FMD_CIQ_S16 rows: `rows_s16` -- feed_spec.mpx16 (saturate(round_half_even(x * 8192)), NaN 0) of both parts.
  `fma32` is a correctly rounded float32 fma on arrays; `chain_complex` / `chain_real` restate the two kernels' MFMA
  chains for one output (k_chan on (v, +0) input against k_chan_real): the same fmas with the terms that are products
  of the zero imaginary branch sums deleted, an odd half padded with fma(+0, +0, acc).
"""
import numpy as np

import chan_spec as cs
from feed_spec import mpx16

F32 = np.float32


def convert(v):
    """FMD_REAL_F32 / _S8 / _S16 samples as the float32 the kernels filter"""
    v = np.asarray(v)
    if v.dtype == np.int8:
        return v.astype(F32) * F32(2.0 ** -7)
    if v.dtype == np.int16:
        return v.astype(F32) * F32(2.0 ** -15)
    assert v.dtype == np.float32, v.dtype
    return v


def pairs(v):
    """[..., n] real samples -> [..., n, 2] float32 (v, +0): the complex twin's input"""
    f = convert(v)
    out = np.zeros(f.shape + (2,), F32)
    out[..., 0] = f
    return out


def truth(v, n_bins, decimation, shifts, **kw):
    return cs.truth(pairs(v).reshape(-1, 2), n_bins, decimation, shifts, **kw)


def reference_rows(v, n_bins, decimation, shifts, **kw):
    return cs.reference_rows(pairs(v).reshape(-1, 2), n_bins, decimation, shifts, **kw)


def rows_s16(rows):
    """complex64 [..., n] -> int16 [..., n, 2]: what a FMD_CIQ_S16 call stores where the FMD_CIQ_F32 call stores rows"""
    r = np.ascontiguousarray(rows, dtype=np.complex64)
    return mpx16(r.view(F32).reshape(r.shape + (2,)))


def fma32(a, b, c):
    """round_to_nearest_even_float32(a * b + c), exactly: the product of two float32 is exact in float64, the sum's
    rounding error is recovered (TwoSum) and decides the one case float64 -> float32 would round twice, a tie"""
    a, b, c = (np.asarray(t, F32).astype(np.float64) for t in np.broadcast_arrays(a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        f = s.astype(F32)
        f64 = f.astype(np.float64)
        g = np.nextafter(f, np.where(s > f64, np.inf, -np.inf).astype(F32))
        tie = np.isfinite(s) & (f64 != s) & ((s - f64) == (g.astype(np.float64) - s)) & (e != 0)
        toward_g = np.sign(e) == np.sign(s - f64)
    return np.where(tie & toward_g, g, f).astype(F32)


def _finish(acc0, acc1, scale2):
    with np.errstate(invalid="ignore", over="ignore"):
        return ((acc0 + acc1).astype(F32) * F32(scale2)).astype(F32)


def chain_complex(W, U, scale2=2.0):
    """k_chan's two outputs (Re y, Im y) [..] for W [N] complex64, U [.., N] float32 real branch sums, Im U = +0: k in
    order 2 r (Re U), 2 r + 1 (Im U); halves [0, N / 2), [N / 2, 2 (N / 2)), for odd N branch N - 1 last on the
    second"""
    W = np.asarray(W, np.complex64)
    U = np.asarray(U, F32)
    N, Nh = W.size, W.size // 2
    zero = np.zeros(U.shape[:-1], F32)
    out = []
    for a_re, a_im in ((W.real, -W.imag), (W.imag, W.real)):  # row 2 b, row 2 b + 1 of A
        acc = [zero.copy(), zero.copy()]
        for half, rs in enumerate((range(0, Nh), list(range(Nh, 2 * Nh)) + ([N - 1] if N & 1 else []))):
            for r in rs:
                acc[half] = fma32(a_re[r], U[..., r], acc[half])
                acc[half] = fma32(a_im[r], zero, acc[half])
        out.append(_finish(acc[0], acc[1], scale2))
    return out


def chain_real(W, U, scale2=2.0):
    """k_chan_real's: the same chains without the Im U terms, two branches an MFMA step, an odd half padded with
    A = U = +0"""
    W = np.asarray(W, np.complex64)
    U = np.asarray(U, F32)
    N, Nh = W.size, W.size // 2
    zero = np.zeros(U.shape[:-1], F32)
    out = []
    for a in (W.real, W.imag):
        acc = [zero.copy(), zero.copy()]
        for half, rs in enumerate((list(range(0, Nh)), list(range(Nh, N)))):
            for r in rs:
                acc[half] = fma32(a[r], U[..., r], acc[half])
            if len(rs) & 1:
                acc[half] = fma32(F32(0.0), zero, acc[half])
        out.append(_finish(acc[0], acc[1], scale2))
    return out


def same_but_zero_signs(a, b):
    """equal bits wherever either is not a zero (NaN matches NaN), zeros compared with =="""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    if a.shape != b.shape:
        return False
    zero = (a == 0) & (b == 0)
    return bool(np.all(zero | (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
