"""A numpy restatement of what one f64 GEMM launch of the engine must compute (``GemmArgs`` in gumbi_amd/csrc/gemm_f64.hpp),
written from the comments of that header and sharing no code with the engine:

    C[nc(i), j] = beta * C0[nc(i), j] + alpha * sum_{k in [k_lo, k_hi)} B[nb(i), k] * A[j, k]        i < n, j < m

* the n index walks 128-row blocks that are ``nblk_stride`` blocks apart in B's memory and ``cblk_stride`` (0 = the same) blocks
  apart in C's:  nb(i) = (i // 128) * nblk_stride * 128 + i % 128;
* the launch works on BM x BN tiles (tm = j // BM, tn = i // BN); per tile
      R    = row(first i of the tile, stride krow_stride or nblk_stride) + krow_off
      k_hi = min(k, R + BN) if khi_n else k
      k_lo = klo_m * tm * BM + klo_n * R, clamped to [0, k_hi]              (an empty range leaves C = beta * C0)
* ``tri``: a tile whose last row nb + BN - 1 + tri_off lies above its first column tm * BM is skipped -- C keeps its bits.

Two independent implementations (tile by tile; per-element index masks) that tests/test_gemm_reference_cpu.py holds against
each other, and the input generators of tests/test_gpu_gemm.py: exactly representable integer operands, standard-normal
operands with a derived rounding bound, NaN poison over everything a kernel has no business reading and a sentinel bit pattern
over everything it has no business writing.

Arrays here are LOGICAL: A is (m, k), B is (rows of B's memory, k), C is (rows of C's memory, m).  `Problem` lays them out in
column-major device-style buffers with leading dimensions, guard bands and offsets.
"""
from dataclasses import dataclass, replace

import numpy as np

U = 2.0 ** -53
#: bit pattern of every C entry the launch must leave alone (finite, so a kernel that reads it into a sum shows up as well)
SENTINEL = np.array([-1234567.140625]).view(np.uint64)[0]
SENTINEL_F = np.array([SENTINEL], dtype=np.uint64).view(np.float64)[0]
GUARD_N = 128   # guard rows before / after every operand along the contiguous index
GUARD_K = 16    # guard k-rows (A, B) before / after
GUARD_M = 128   # guard columns of C before / after


@dataclass(frozen=True)
class Desc:
    m: int
    n: int
    k: int
    alpha: float = 1.0
    beta: float = 0.0
    tri: int = 0
    tri_off: int = 0
    nblk_stride: int = 1
    cblk_stride: int = 0
    klo_m: int = 0
    klo_n: int = 0
    khi_n: int = 0
    krow_off: int = 0
    krow_stride: int = 0

    @property
    def b_rows(self):
        return ((self.n // 128 - 1) * max(1, self.nblk_stride) + 1) * 128

    @property
    def c_rows(self):
        return ((self.n // 128 - 1) * (self.cblk_stride or max(1, self.nblk_stride)) + 1) * 128


def noff(tn, bn, stride):
    """Memory row of the first row of n-tile ``tn`` (tile height bn <= 128) under a block stride."""
    e = tn * bn
    return (e // 128) * stride * 128 + e % 128


# ---- implementation 1: tile by tile -----------------------------------------------------------------------------------------
def reference_tiles(A, B, C0, d, BM, BN, dtype=np.float64):
    """(C, written, k_eff): the expected C (same shape as C0; entries outside `written` are C0's), the mask of entries the launch
    must have written, and the contraction length behind every written entry."""
    sb = max(1, d.nblk_stride)
    sc = d.cblk_stride or sb
    sk = d.krow_stride or sb
    A = np.asarray(A, dtype=dtype)
    B = np.asarray(B, dtype=dtype)
    C = np.array(C0, dtype=dtype)
    written = np.zeros(C.shape, dtype=bool)
    keff = np.zeros(C.shape, dtype=np.int64)
    alpha, beta = dtype(d.alpha), dtype(d.beta)
    for tm in range(d.m // BM):
        for tn in range(d.n // BN):
            nb, nc = noff(tn, BN, sb), noff(tn, BN, sc)
            if d.tri and nb + BN - 1 + d.tri_off < tm * BM:
                continue
            R = noff(tn, BN, sk) + d.krow_off
            k_hi = min(d.k, R + BN) if d.khi_n else d.k
            k_lo = min(max(d.klo_m * tm * BM + d.klo_n * R, 0), k_hi)
            rows, cols = slice(nc, nc + BN), slice(tm * BM, (tm + 1) * BM)
            if k_hi > k_lo:
                acc = B[nb:nb + BN, k_lo:k_hi] @ A[cols, k_lo:k_hi].T
            else:
                acc = np.zeros((BN, BM), dtype=dtype)
            C[rows, cols] = alpha * acc if d.beta == 0 else beta * C[rows, cols] + alpha * acc
            written[rows, cols] = True
            keff[rows, cols] = max(k_hi - k_lo, 0)
    return C, written, keff


# ---- implementation 2: per-element index masks ------------------------------------------------------------------------------
def reference_masks(A, B, C0, d, BM, BN, dtype=np.float64):
    """The same three results from index arithmetic over whole arrays: no loop over tiles, no slicing of k ranges (finite
    operands only)."""
    sb = max(1, d.nblk_stride)
    sc = d.cblk_stride or sb
    sk = d.krow_stride or sb
    i = np.arange(d.n)
    j = np.arange(d.m)
    kk = np.arange(d.k)

    def row(idx, stride):
        return idx // 128 * 128 * stride + idx % 128

    first = i - i % BN                               # first logical n index of the element's tile
    rb, rc = row(i, sb), row(i, sc)
    R = row(first, sk) + d.krow_off                  # (n,)
    col0 = j - j % BM                                # tm * BM, (m,)
    skipped = (d.tri != 0) & ((row(first, sb) + BN - 1 + d.tri_off)[:, None] < col0[None, :])
    k_hi = np.minimum(d.k, R + BN) if d.khi_n else np.full(d.n, d.k)
    k_lo = d.klo_m * col0[None, :] + d.klo_n * R[:, None]
    k_lo = np.minimum(np.maximum(k_lo, 0), k_hi[:, None])               # (n, m)
    Bz = np.asarray(B, dtype=dtype)[rb]              # (n, k) in logical order; finite operands only (no poison here)
    Az = np.asarray(A, dtype=dtype)
    Bz = np.where(kk[None, :] < k_hi[:, None], Bz, dtype(0))
    acc = np.zeros((d.n, d.m), dtype=dtype)
    for v in np.unique(k_lo):                        # one masked product per distinct lower end
        keep = kk[None, :] >= v
        acc = np.where(k_lo == v, np.where(keep, Bz, dtype(0)) @ np.where(keep, Az, dtype(0)).T, acc)
    length = np.maximum(k_hi[:, None] - k_lo, 0)
    C = np.array(C0, dtype=dtype)
    old = C[rc]
    new = dtype(d.alpha) * acc if d.beta == 0 else dtype(d.beta) * old + dtype(d.alpha) * acc
    C[rc] = np.where(skipped, old, new)
    written = np.zeros(C.shape, dtype=bool)
    written[rc] = ~skipped
    keff = np.zeros(C.shape, dtype=np.int64)
    keff[rc] = np.where(skipped, 0, length)
    return C, written, keff


def gamma(nn):
    """gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, ch. 3)."""
    nn = np.asarray(nn, dtype=np.float64)
    return nn * U / (1.0 - nn * U)


def rounding_bound(A, B, C0, d, BM, BN):
    """Entrywise bound on |float64 result - exact| for ANY summation order, with or without FMA: a dot product of length k_eff
    carries at most gamma_{k_eff} relative to sum |a||b|; the multiplications by alpha and beta and the final addition add
    three more roundings -- gamma_{k_eff + 3} * (|alpha| |B| |A|^T over the tile's k range + |beta| |C0|), evaluated in long
    double.  NaN poison must be outside the ranges read (it is, by construction)."""
    da = replace(d, alpha=abs(d.alpha), beta=abs(d.beta))
    C0a = np.abs(np.where(np.isfinite(C0), C0, 0.0))
    mag, written, keff = reference_tiles(np.abs(A), np.abs(B), C0a, da, BM, BN, dtype=np.longdouble)
    return (gamma(keff + 3).astype(np.longdouble) * mag).astype(np.float64), written


# ---- inputs -----------------------------------------------------------------------------------------------------------------
class Problem:
    """Operands of one launch in column-major buffers, the way the engine sees them:

        bufA (GUARD_K + k + GUARD_K, lda)   A[j, k]  at bufA[GUARD_K + k, GUARD_N + j]
        bufB (GUARD_K + k + GUARD_K, ldb)   B[r, k]  at bufB[GUARD_K + k, GUARD_N + r]
        bufC (GUARD_M + m + GUARD_M, ldc)   C[r, j]  at bufC[GUARD_M + j, GUARD_N + r]

    (row-major numpy / torch arrays of the transposed shape).  Everything of bufA / bufB outside what the launch may read is NaN;
    everything of bufC outside what it must write holds SENTINEL.  ``pbm, pbn`` = the tile shape the poison is cut for (128, 128
    when the tile shape is left to the launcher: safe for every shape).  In place (``in_place``): bufC is bufB."""

    def __init__(self, d, pbm, pbn, kind="exact", seed=0, in_place=False, pad=(64, 192, 320)):
        rng = np.random.default_rng(seed)
        self.d, self.pbm, self.pbn, self.in_place = d, pbm, pbn, in_place
        draw = (lambda shape: rng.integers(-8, 9, size=shape).astype(np.float64)) if kind == "exact" else rng.standard_normal
        sb = max(1, d.nblk_stride)
        sk = d.krow_stride or sb
        self.lda = GUARD_N + d.m + GUARD_N + pad[0]
        self.ldb = GUARD_N + d.b_rows + GUARD_N + pad[1]
        self.ldc = self.ldb if in_place else GUARD_N + d.c_rows + GUARD_N + pad[2]
        # logical operands with the poison in
        kk = np.arange(d.k)
        A = draw((d.m, d.k))
        if d.klo_m:
            j = np.arange(d.m)
            A[kk[None, :] < (j - j % pbm)[:, None]] = np.nan
        B = np.full((d.b_rows, d.k), np.nan)
        for tn in range(d.n // pbn):
            nb = noff(tn, pbn, sb)
            blk = draw((pbn, d.k))
            R = noff(tn, pbn, sk) + d.krow_off
            if d.klo_n:
                blk[:, kk < R] = np.nan
            if d.khi_n:
                blk[:, kk >= R + pbn] = np.nan
            B[nb:nb + pbn] = blk
        self.A, self.B = A, B
        self.C0_values = draw((d.c_rows, d.m))  # what C holds wherever the launch writes (beta != 0)
        self.bufA = np.full((2 * GUARD_K + d.k, self.lda), np.nan)
        self.bufA[GUARD_K:GUARD_K + d.k, GUARD_N:GUARD_N + d.m] = A.T
        self.bufB = np.full((2 * GUARD_K + d.k, self.ldb), np.nan)
        self.bufB[GUARD_K:GUARD_K + d.k, GUARD_N:GUARD_N + d.b_rows] = B.T
        self.offA = GUARD_K * self.lda + GUARD_N
        self.offB = GUARD_K * self.ldb + GUARD_N
        self.offC = self.offB if in_place else GUARD_M * self.ldc + GUARD_N

    def c_buffer(self, BM, BN):
        """bufC for a launch that runs BM x BN tiles, and the logical C0 inside it: SENTINEL wherever that launch must not write,
        NaN (beta == 0: C must not be read) or random values where it must."""
        d = self.d
        _, must, _ = reference_tiles(np.zeros((d.m, d.k)), np.zeros((d.b_rows, d.k)), np.zeros((d.c_rows, d.m)),
                                     replace(d, alpha=1.0, beta=1.0), BM, BN)
        C0 = np.where(must, np.nan if d.beta == 0 else self.C0_values, SENTINEL_F)
        buf = np.full((2 * GUARD_M + d.m, self.ldc), SENTINEL_F)
        buf[GUARD_M:GUARD_M + d.m, GUARD_N:GUARD_N + d.c_rows] = C0.T
        return buf, C0, must

    def check_in_place(self, got_buf):
        """The in-place form (C is B, m == k == 128, beta == 0): rows of the n range hold alpha * B A^T exactly, every other
        entry of the buffer -- guard rows, guard k-rows, the rows between strided blocks -- keeps its bits."""
        d = self.d
        assert self.in_place and d.m == d.k and d.beta == 0 and not (d.tri or d.klo_m or d.klo_n or d.khi_n)
        want = self.bufB.copy()
        rows = np.concatenate([np.arange(128) + noff(t, 128, max(1, d.nblk_stride)) for t in range(d.n // 128)])
        prod = d.alpha * (self.B[rows] @ self.A.T)  # (n, m)
        assert np.isfinite(prod).all(), "test bug: the reference reads poison"
        written = np.zeros(want.shape, dtype=bool)
        written[GUARD_K:GUARD_K + d.m, GUARD_N + rows] = True
        want[GUARD_K:GUARD_K + d.m, GUARD_N + rows] = prod.T
        same = np.ascontiguousarray(got_buf).view(np.uint64) == want.view(np.uint64)
        assert same[~written].all(), f"{int((~same[~written]).sum())} entries outside the product's rows changed"
        ok = got_buf[written] == want[written]
        assert ok.all(), f"{int((~ok).sum())} of {int(written.sum())} entries differ"

    def unpack_c(self, buf):
        return buf[GUARD_M:GUARD_M + self.d.m, GUARD_N:GUARD_N + self.d.c_rows].T

    def check(self, got_buf, BM, BN, kind="exact"):
        """Assert the launch's result: written entries equal the reference (bit for bit on exact inputs, inside the derived bound on
        real ones), every other entry of the whole buffer still holds SENTINEL's bits."""
        d = self.d
        buf0, C0, must = self.c_buffer(BM, BN)
        got = self.unpack_c(got_buf)
        untouched = np.ones(got_buf.shape, dtype=bool)
        untouched[GUARD_M:GUARD_M + d.m, GUARD_N:GUARD_N + d.c_rows] = ~must.T
        bits = np.ascontiguousarray(got_buf).view(np.uint64)
        bad = untouched & (bits != SENTINEL)
        assert not bad.any(), f"{int(bad.sum())} entries outside the launch's tiles were written, first at (m, row) {np.argwhere(bad)[0] - (GUARD_M, GUARD_N)}"
        if kind == "exact":
            want, _, _ = reference_tiles(self.A, self.B, C0, d, BM, BN)
            assert np.isfinite(want[must]).all(), "test bug: the reference reads poison"
            ok = got[must] == want[must]
            assert ok.all(), (f"{int((~ok).sum())} of {int(must.sum())} entries differ, first at (row, m) "
                              f"{np.argwhere(must & (got != want))[0]}: got {got[must][~ok][0]!r}, want {want[must][~ok][0]!r}")
        else:
            want, _, _ = reference_tiles(self.A, self.B, C0, d, BM, BN, dtype=np.longdouble)
            bound, _ = rounding_bound(self.A, self.B, C0, d, BM, BN)
            err = np.abs((got.astype(np.longdouble) - want)[must]).astype(np.float64)
            assert np.isfinite(got[must]).all(), "NaN / Inf in the result: an operand was read outside its range"
            worst = float(np.max(err / np.maximum(bound[must], 1e-300)))
            print(f"  max |got - ref| / bound = {worst:.3f}")
            assert (err <= bound[must]).all(), f"error exceeds the gamma bound by a factor {worst:.3g}"


def exact_premise_holds(k, seed=0):
    """Integers in [-8, 8], k <= 4096: |sum| <= 64 * 4096 = 2^18, times |alpha| <= 2 plus |beta| * 8 -- every partial result in
    any order is an integer (or a half-integer for the 0.5 scalars) far below 2^53: float64, long double and int64 agree."""
    rng = np.random.default_rng(seed)
    a = rng.integers(-8, 9, size=(64, k))
    b = rng.integers(-8, 9, size=(96, k))
    a[0], b[0] = 8, -8  # the extreme sum
    exact = b @ a.T
    f64 = b.astype(np.float64) @ a.astype(np.float64).T
    ld = b.astype(np.longdouble) @ a.astype(np.longdouble).T
    return np.array_equal(f64, exact) and np.array_equal(ld, exact) and abs(exact).max() == 64 * k
