"""The channeliser kernels' arithmetic in numpy, bit for bit: what tests/test_chan_model_cpu.py proves right on the CPU
and tests/test_gpu_chan_shapes.py holds the device's rows against.  Restated from the text of csrc/fmd_k_chan.hip.h
(k_chan, k_chan_real) and of chan_upload_table / chan_twiddles (csrc/fmd_chan.inc.hpp); nothing here calls the library.

  taps       chan_spec.taps(K, cutoff): c[1 .. K]
  history    x[q] = +0 for q < 0
  branch     u_q[r], q a multiple of D: one fma32(c[j], x[q - j], u) per tap and part from +0, j ascending from the
  sums       first j in 1 .. N with (q - j) = r (mod N), step N, while j <= K; a branch with no tap stays +0.  A real
             capture has one plane.
  twiddles   W[r] = exp(+2 pi i ((s mod N) r mod N) / N): the angle in double, cos and sin of the C library rounded
             once to float32
  bins       row b of a capture owns rows 2 b (Re y) and 2 b + 1 (Im y) of A.  Complex: row 2 b is (Wre, -Wim), row
             2 b + 1 is (Wim, Wre) over k = 2 r + part, U's k = 2 r is Re u[r], k = 2 r + 1 is Im u[r]; one accumulator
             takes r in [0, N / 2), a second [N / 2, N) (so branch N - 1 of an odd N comes last on the second), each
             from +0 with one fma32 per k in k order.  Real: the same without the Im u products; a half with an odd
             number of branches ends with fma32(+0, +0, acc).
  finish     float32(acc0 + acc1) * float32(2 out_scale), rounded to float32

The model holds for finite input whose products and sums are all normal numbers or zeros (how the matrix cores treat
subnormals is not modelled): `run` returns, beside the rows, the smallest non-zero magnitude among all products and
sums it formed, and the tests assert that it is a normal float32.

`wrong=` selects a deliberately faulty variant, for the tests that show which rows each fault would change:
  "drop_tap_k"   tap K is left out of the branch sums
  "ignore_qm"    branch r starts at the j of q = 0 at every output time (q mod N ignored)
  "split_up"     the halves split at (N + 1) / 2 instead of N / 2
  "row_xor_1"    row b's twiddles sit in row b ^ 1 of its block
  "block_0"      every row block reads block 0's table (row b gets the twiddles of row b mod 16)
"""
import collections
import hashlib
import math

import numpy as np

import chan_real_spec as crs
import chan_spec as cs

F32 = np.float32
TINY = float(np.finfo(F32).tiny)
WRONG = ("drop_tap_k", "ignore_qm", "split_up", "row_xor_1", "block_0")
ROWS_PER_BLOCK = 16

Result = collections.namedtuple("Result", "rows floor U")


class _Fma:
    """fma32 that keeps the smallest non-zero |product| and |result| it met"""

    def __init__(self):
        self.floor = np.inf

    def note(self, v, mask=None):
        a = np.abs(np.asarray(v, np.float64))
        if mask is not None:
            a = a[np.broadcast_to(mask, a.shape)]
        a = a[a > 0]
        if a.size:
            self.floor = min(self.floor, float(a.min()))

    def __call__(self, a, b, c, mask=None):
        a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
        out = crs.fma32(a, b, c)
        self.note(a.astype(np.float64) * b.astype(np.float64), mask)
        self.note(out, mask)
        return out


_twiddle_cache = {}


def twiddles(N, shift):
    """(Wre [N], Wim [N]) float32 as chan_twiddles makes them (math.cos / math.sin: the C library's, as the host's)"""
    N = int(N)
    s = int(shift) % N
    if (N, s) not in _twiddle_cache:
        ang = [2.0 * math.pi * float((s * r) % N) / float(N) for r in range(N)]
        _twiddle_cache[N, s] = (np.array([math.cos(a) for a in ang], np.float64).astype(F32),
                                np.array([math.sin(a) for a in ang], np.float64).astype(F32))
    return _twiddle_cache[N, s]


def planes(x, real):
    """the capture as float32 planes [parts, n]: one plane of a real capture, (I, Q) of a complex one"""
    if real:
        v = np.ascontiguousarray(crs.convert(np.asarray(x))).reshape(1, -1)
        return v
    x = np.asarray(x)
    assert x.dtype in (np.float32, np.complex64), x.dtype
    p = np.ascontiguousarray(x).view(F32).reshape(-1, 2)
    return np.ascontiguousarray(p.T)


_sums_cache = {}


def branch_sums(x, n_bins, decimation, filter_order, real=False, cutoff=0.0, wrong=None):
    """(U [parts, outputs, N] float32, floor): step 2 of the kernels over one capture's whole stream from q = 0,
    memoised per stream and geometry"""
    N, D, K = int(n_bins), int(decimation), int(filter_order)
    cutoff = float(cutoff) or 0.6 / D
    p = planes(x, real)
    key = (hashlib.sha1(p.tobytes()).hexdigest(), p.shape, N, D, K, cutoff, wrong if wrong in WRONG[:2] else None)
    if key in _sums_cache:
        return _sums_cache[key]
    c = cs.taps(K, cutoff)
    assert c.shape == (K + 1,) and c.dtype == F32
    n = p.shape[1]
    q = np.arange(0, n, D, dtype=np.int64)                                  # the output times
    xp = np.concatenate([np.zeros((p.shape[0], K), F32), p], axis=1)         # xp[:, K + i] = x[i]; +0 in front
    r = np.arange(N, dtype=np.int64)
    j0 = ((0 if wrong == "ignore_qm" else q[:, None]) - r[None, :]) % N
    j0 = np.broadcast_to(np.where(j0 == 0, N, j0), (q.size, N))              # the first tap: 1 <= j0 <= N
    last = K - 1 if wrong == "drop_tap_k" else K
    fma = _Fma()
    U = np.zeros((p.shape[0], q.size, N), F32)
    for i in range(0, (K + N - 1) // N + 1):
        j = j0 + i * N
        valid = j <= last
        if not valid.any():
            break
        jc = np.minimum(j, K)
        cj = c[jc]
        for part in range(p.shape[0]):
            xs = xp[part][K + q[:, None] - jc]
            U[part] = np.where(valid, fma(cj, xs, U[part], mask=valid), U[part])
    _sums_cache[key] = (U, fma.floor)
    return _sums_cache[key]


def table_shifts(shifts, wrong=None):
    """which shift's twiddles the rows of A of row b hold (None: the zeros of an unused slot): row b fills slot b mod
    16 of block b / 16, as chan_upload_table places it"""
    sh = [int(s) for s in shifts]
    B = len(sh)
    out = []
    for b in range(B):
        block, slot = b // ROWS_PER_BLOCK, b % ROWS_PER_BLOCK
        if wrong == "block_0":
            block = 0
        if wrong == "row_xor_1":
            slot ^= 1
        src = block * ROWS_PER_BLOCK + slot
        out.append(sh[src] if src < B else None)
    return out


def half_chains(N, real, wrong=None):
    """the k of the two accumulators, in order; k = nk (one behind the last) is the padded k: A = U = +0.  Complex:
    k = 2 r + part of nk = 2 N; real: k = r of nk = N"""
    Nh = (N + 1) // 2 if wrong == "split_up" else N // 2
    if not real:
        return list(range(0, 2 * Nh)), list(range(2 * Nh, 2 * N))
    pad = [N]
    h0, h1 = list(range(0, Nh)), list(range(Nh, N))
    return h0 + (pad if len(h0) & 1 else []), h1 + (pad if len(h1) & 1 else [])


def bins(U, n_bins, shifts, real=False, out_scale=1.0, wrong=None):
    """(rows [B, outputs] complex64, floor): steps 3 and 4 on the branch sums U [parts, outputs, N]"""
    N = int(n_bins)
    B, O = len(shifts), U.shape[1]
    nk = N if real else 2 * N
    A = np.zeros((2, B, nk + 1), F32)                        # [Re y row / Im y row][b][k], the padded k behind
    for b, s in enumerate(table_shifts(shifts, wrong)):
        if s is None:
            continue
        wre, wim = twiddles(N, s)
        if real:
            A[0, b, :N], A[1, b, :N] = wre, wim
        else:
            A[0, b, 0:nk:2], A[0, b, 1:nk:2] = wre, -wim
            A[1, b, 0:nk:2], A[1, b, 1:nk:2] = wim, wre
    Uk = np.zeros((nk + 1, O), F32)                          # [k][output]
    if real:
        Uk[:N] = U[0].T
    else:
        Uk[0:nk:2], Uk[1:nk:2] = U[0].T, U[1].T
    h0, h1 = half_chains(N, real, wrong)
    fma = _Fma()
    acc = np.zeros((2, 2, B, O), F32)                        # [half][row of the pair][b][output]
    both = min(len(h0), len(h1))
    for i in range(both):
        kk = [h0[i], h1[i]]
        acc = fma(A[:, :, kk].transpose(2, 0, 1)[..., None], Uk[kk][:, None, None, :], acc)
    for h, ks in ((0, h0), (1, h1)):
        for k in ks[both:]:
            acc[h] = fma(A[:, :, k][..., None], Uk[k][None, None, :], acc[h])
    scale2 = F32(F32(2.0) * F32(out_scale))
    s = (acc[0] + acc[1]).astype(F32)
    y = (s * scale2).astype(F32)
    fma.note(s)
    fma.note(y)
    rows = np.empty((B, O), np.complex64)
    rows.real, rows.imag = y[0], y[1]
    return rows, fma.floor


def run(x, n_bins, decimation, filter_order, shifts, real=False, out_scale=1.0, cutoff=0.0, wrong=None):
    """Result(rows [B, outputs] complex64, floor, U): one capture's whole stream from q = 0.  x: float32 [n, 2] or
    complex64 [n]; a real capture: float32 / int8 / int16 [n]."""
    assert wrong is None or wrong in WRONG, wrong
    U, f0 = branch_sums(x, n_bins, decimation, filter_order, real, cutoff, wrong)
    rows, f1 = bins(U, n_bins, shifts, real, out_scale, wrong)
    return Result(rows, min(f0, f1), U)


def rows(x, n_bins, decimation, filter_order, shifts, real=False, out_scale=1.0):
    """[rows, outputs] complex64: the bits the kernels store for one capture's whole stream from q = 0"""
    return run(x, n_bins, decimation, filter_order, shifts, real, out_scale).rows


def rows_s16(r):
    """FMD_CIQ_S16 rows of those rows: [rows, outputs, 2] int16"""
    return crs.rows_s16(r)


def normal(floor):
    """the model's precondition: nothing it formed was a subnormal"""
    return floor >= TINY


# ---------------------------------------------------------------------------------------------------------------
# the shapes both test files use: geometries (N, D, K), streams, shift lists, call sizes

EDGE = [(2, 2, 5), (3, 2, 7), (4, 2, 9), (5, 3, 11), (8, 3, 2), (9, 4, 32), (255, 100, 800), (256, 128, 1024),
        (64, 256, 600), (16, 2, 4096)]
REAL_EDGE = [(2, 2, 5), (3, 2, 7), (5, 3, 11), (511, 230, 1840)]
MANY = [(24, 11, 88), (192, 88, 704)]


def geom_id(g):
    return "N%dD%dK%d" % tuple(g)


def stream_samples(D):
    return 200 * D + 7


def capture(g, n, seed=0, real=False):
    """capture g of a stream: 0.3 x standard normal float32, [n, 2] or [n] real samples, seeded per capture"""
    rng = np.random.default_rng(1000 * seed + g)
    return (rng.standard_normal(n if real else (n, 2)) * 0.3).astype(F32)


def anchor_shifts(N):
    """the 3 x 5 shifts of tests/test_gpu_chan.py: 0, N / 2, negatives, beyond +-N, a duplicate inside a capture"""
    return np.array([[0, N // 2, -1, 3, -(N // 3)],
                     [N // 2, 1, -2, N + 5, 0],
                     [-(N // 2), 2, 2, -N - 1, 7]], np.int32)


def shift_list(N, g, B):
    """B shifts of capture g: distinct residues in a seeded order -- every residue 0 .. N - 1 where B > N, the rest of
    the list then random --, every third entry moved down by N (negatives), every fifth up by 2 N (beyond +-N), and
    the last entry a copy of entry 1 (the one duplicate pair among the first N + 1: for B above 16 in two blocks)"""
    rng = np.random.default_rng(7919 * N + g)
    if B > N:
        vals = list(rng.permutation(N)) + list(rng.integers(0, N, B - N))
    else:
        vals = list(rng.permutation(N)[:B])
    vals = [int(v) for v in vals]
    for i in range(B):
        if i % 3 == 2:
            vals[i] -= N
        if i % 5 == 4:
            vals[i] += 2 * N
    if B > 2:
        vals[B - 1] = vals[1]
    return vals


def shifts(N, G, B):
    return np.array([shift_list(N, g, B) for g in range(G)], np.int32)


_case_cache = {}


def case(geom, G, B, real=False, out_scale=1.0, shift_rows=None):
    """(x [G, n(, 2)], shifts [G, B], model rows [G, B, outputs] complex64, floor) of a G x B channeliser over the
    geometry's stream, memoised.  shift_rows: the shifts, if not shifts(N, G, B)"""
    N, D, K = geom
    sh = shifts(N, G, B) if shift_rows is None else np.asarray(shift_rows, np.int32).reshape(G, B)
    key = (tuple(geom), G, B, bool(real), float(out_scale), sh.tobytes())
    if key not in _case_cache:
        x = np.stack([capture(g, stream_samples(D), 0, real) for g in range(G)])
        res = [run(x[g], N, D, K, sh[g], real=real, out_scale=out_scale) for g in range(G)]
        want = np.stack([r.rows for r in res])
        want.setflags(write=False)
        _case_cache[key] = (x, sh, want, min(r.floor for r in res))
    return _case_cache[key]


def call_sizes(D, K):
    """one stream of ragged calls: 1, around D, K, around the kernel's tile of 32 outputs, the rest"""
    total = stream_samples(D)
    return cs.ragged(total, [1, D - 1, D + 1, K, 32 * D - 1, 32 * D, 32 * D + 1, total])


# ---------------------------------------------------------------------------------------------------------------
# the comparison both test files use

def _parts(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.complex64:
        return a.view(F32).reshape(a.shape + (2,))
    assert a.dtype in (np.int16, np.float32) and a.shape[-1] == 2, (a.dtype, a.shape)
    return a


def first_difference(got, want, zero_signs=False):
    """index of the first output of a row [outputs] (complex64, or [outputs, 2] int16) whose bits are not the wanted
    ones -- zero_signs: a zero matches a zero of either sign -- or None"""
    g, w = _parts(got), _parts(want)
    if g.shape != w.shape or g.dtype != w.dtype:
        return 0
    if g.dtype == np.float32:
        eq = g.view(np.uint32) == w.view(np.uint32)
        if zero_signs:
            eq |= (g == 0) & (w == 0)
    else:
        eq = g == w
    bad = np.flatnonzero(~eq.all(axis=-1))
    return int(bad[0]) if bad.size else None


def row_faults(got, want, what, zero_signs=False):
    """got, want: [G, B, outputs] complex64 (or [G, B, outputs, 2] int16).  One line per row that differs: geometry and
    shape (what), capture, row, the first differing output, and whether the row is the model's row of another (g, b) --
    the signature of a table or row-mapping fault"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    G, B = want.shape[:2]
    out = []
    for g in range(G):
        for b in range(B):
            at = first_difference(got[g, b], want[g, b], zero_signs)
            if at is None:
                continue
            twin = [(h, c) for h in range(G) for c in range(B)
                    if (h, c) != (g, b) and first_difference(got[g, b], want[h, c], zero_signs) is None]
            line = "%s: capture %d row %d differs from the model first at output %d (got %r, model %r)" % (
                what, g, b, at, got[g, b][at].tolist(), want[g, b][at].tolist())
            line += "; it IS the model's row of (capture, row) %s" % twin if twin else "; it is no other row of the model"
            out.append(line)
    return out


def assert_rows(got, want, what, zero_signs=False):
    faults = row_faults(got, want, what, zero_signs)
    assert not faults, "%d of %d rows differ\n%s" % (len(faults), want.shape[0] * want.shape[1], "\n".join(faults[:12]))
