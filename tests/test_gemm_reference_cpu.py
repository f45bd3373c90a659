"""The numpy restatement of the GEMM launch semantics (tests/gemm_reference.py) against itself: its two implementations agree on
a grid of small descriptors that covers every field, both reduce to the plain product when no option is set, the exact-input
premise holds at the largest k in use, and the derived rounding bound admits numpy's own float64 product but not a product with
one k-slice of 4 missing.  Runs everywhere (no GPU)."""
import itertools
from dataclasses import replace

import numpy as np
import pytest

import gemm_reference as GR
from gemm_reference import Desc

SHAPES = [(128, 128), (64, 64), (128, 64), (128, 32)]


def _dense_inputs(d, seed, kind="exact"):
    rng = np.random.default_rng(seed)
    draw = (lambda s: rng.integers(-8, 9, size=s).astype(np.float64)) if kind == "exact" else rng.standard_normal
    return draw((d.m, d.k)), draw((d.b_rows, d.k)), draw((d.c_rows, d.m))


def _grid():
    base = Desc(m=256, n=256, k=256, alpha=-1.0, beta=1.0)
    out = [base, replace(base, alpha=2.0, beta=0.0), replace(base, m=128, n=384, alpha=0.5, beta=-1.0)]
    for off in (0, 128, -128, 64, -64, 32):
        out.append(replace(base, tri=1, tri_off=off))
        out.append(replace(base, m=384, n=256, tri=1, tri_off=off))
    for f in itertools.product((0, 1), repeat=3):
        out.append(replace(base, klo_m=f[0], klo_n=f[1], khi_n=f[2]))
    for off in (128, -128):
        out.append(replace(base, klo_n=1, krow_off=off))
        out.append(replace(base, khi_n=1, krow_off=off, beta=0.0))
        out.append(replace(base, klo_n=1, khi_n=1, krow_off=off))
    for ks in (2, 3):
        out.append(replace(base, klo_n=1, krow_stride=ks, k=512))
        out.append(replace(base, khi_n=1, krow_stride=ks, krow_off=-128, k=512))
    for s, c in itertools.product((2, 3), (0, 1)):
        out.append(replace(base, nblk_stride=s, cblk_stride=c))
        out.append(replace(base, nblk_stride=s, cblk_stride=c, tri=1, tri_off=128, m=384, k=128))
        out.append(replace(base, nblk_stride=s, cblk_stride=c, klo_n=1, krow_off=128, krow_stride=0, k=640, beta=0.0))
        out.append(replace(base, nblk_stride=1, cblk_stride=c * 2, klo_n=1, krow_off=128, krow_stride=s, k=640))
        # the memory stride and the logical stride both in play and different: R(tn) is not noff(tn) + krow_off
        out.append(replace(base, nblk_stride=s, cblk_stride=c, klo_n=1, krow_off=128, krow_stride=5 - s, k=640))
        out.append(replace(base, nblk_stride=s, cblk_stride=c, klo_n=1, khi_n=1, krow_off=128, krow_stride=5 - s, k=640))
    out.append(replace(base, m=384, klo_m=1, k=256))  # the last m-tiles' range is empty
    return out


@pytest.mark.parametrize("bm,bn", SHAPES)
def test_tile_and_mask_implementations_agree(bm, bn):
    for idx, d in enumerate(_grid()):
        A, B, C0 = _dense_inputs(d, idx)
        c1, w1, k1 = GR.reference_tiles(A, B, C0, d, bm, bn)
        c2, w2, k2 = GR.reference_masks(A, B, C0, d, bm, bn)
        assert np.array_equal(w1, w2), d
        assert np.array_equal(k1, k2), d
        assert np.array_equal(c1, c2), d  # exact inputs: bit for bit
        assert np.array_equal(c1[~w1], C0[~w1])


@pytest.mark.parametrize("bm,bn", SHAPES)
def test_no_option_is_the_plain_product(bm, bn):
    for (m, n, k), (alpha, beta) in itertools.product([(128, 128, 16), (256, 384, 144), (384, 256, 80)],
                                                      [(-1, 1), (2, 0), (0.5, -1), (1, 0.5), (0, 1)]):
        d = Desc(m=m, n=n, k=k, alpha=alpha, beta=beta)
        A, B, C0 = _dense_inputs(d, m + k)
        want = C0 * beta + alpha * B @ A.T
        for f in (GR.reference_tiles, GR.reference_masks):
            c, w, keff = f(A, B, C0, d, bm, bn)
            assert w.all() and (keff == k).all() and np.array_equal(c, want)


def test_empty_ranges_and_skipped_tiles_by_hand():
    """Three values worked out by hand from the header's comments, so that the two implementations cannot agree on a shared
    misreading: 64 x 64 tiles, tri_off = -64 skips tile (tm, tn) when tn*64 + 63 - 64 < tm*64, i.e. tn <= tm (tm >= 1) ...; khi_n
    with krow_off = -128 gives the first 128 rows k_hi <= 0: C = beta * C0 there; klo_m with tm*BM >= k: the same."""
    d = Desc(m=256, n=256, k=128, alpha=1.0, beta=2.0, tri=1, tri_off=-64)
    A, B, C0 = _dense_inputs(d, 1)
    _, w, _ = GR.reference_tiles(A, B, C0, d, 64, 64)
    tiles = {(tm, tn) for tm in range(4) for tn in range(4) if w[tn * 64, tm * 64]}
    assert tiles == {(tm, tn) for tm in range(4) for tn in range(4) if tn * 64 - 1 >= tm * 64}
    d = Desc(m=128, n=256, k=128, alpha=1.0, beta=2.0, khi_n=1, krow_off=-128)
    A, B, C0 = _dense_inputs(d, 2)
    c, w, keff = GR.reference_tiles(A, B, C0, d, 128, 32)
    assert w.all() and (keff[:128] == 0).all() and np.array_equal(c[:128], 2.0 * C0[:128])
    assert [int(keff[r, 0]) for r in (128, 160, 192, 224)] == [32, 64, 96, 128]
    d = Desc(m=384, n=128, k=256, alpha=1.0, beta=0.0, klo_m=1)
    A, B, C0 = _dense_inputs(d, 3)
    c, w, keff = GR.reference_masks(A, B, C0, d, 128, 64)
    assert w.all() and (keff[:, 256:] == 0).all() and (c[:, 256:] == 0).all() and (keff[:, 128:256] == 128).all()


def test_exact_inputs_are_exact_at_the_largest_k():
    assert GR.exact_premise_holds(4096)
    assert GR.exact_premise_holds(1040, seed=1)


@pytest.mark.parametrize("bm,bn", SHAPES)
def test_rounding_bound_admits_float64_and_rejects_a_missing_slice(bm, bn):
    cases = [Desc(m=256, n=384, k=144, alpha=-1.0, beta=1.0), Desc(m=128, n=128, k=1040, alpha=0.5, beta=-1.0),
             Desc(m=256, n=256, k=256, alpha=2.0, beta=0.0, klo_n=1, khi_n=1), Desc(m=128, n=256, k=16, alpha=1.0, beta=0.5),
             Desc(m=256, n=256, k=640, alpha=1.0, beta=1.0, nblk_stride=2, cblk_stride=1, klo_n=1, krow_off=128, tri=1, tri_off=128)]
    for idx, d in enumerate(cases):
        A, B, C0 = _dense_inputs(d, 10 + idx, kind="real")
        ref, w, keff = GR.reference_tiles(A, B, C0, d, bm, bn, dtype=np.longdouble)
        bound, w2 = GR.rounding_bound(A, B, C0, d, bm, bn)
        assert np.array_equal(w, w2)
        f64, _, _ = GR.reference_tiles(A, B, C0, d, bm, bn)
        err = np.abs((f64.astype(np.longdouble) - ref)[w]).astype(np.float64)
        assert (err <= bound[w]).all(), d
        # one k-slice of 4 dropped from every tile (the first 4 of each tile's own range): far outside the bound somewhere
        A2 = A.copy()
        bad = f64.copy()
        for tm in range(d.m // bm):
            for tn in range(d.n // bn):
                one = replace(d, m=bm, n=bn, tri=0, nblk_stride=1, cblk_stride=0, krow_stride=0, klo_m=0,
                              krow_off=GR.noff(tn, bn, d.krow_stride or d.nblk_stride) + d.krow_off)
                nb, nc = GR.noff(tn, bn, d.nblk_stride), GR.noff(tn, bn, d.cblk_stride or d.nblk_stride)
                if not w[nc, tm * bm] or keff[nc, tm * bm] < 4:
                    continue
                k_lo = min(max(d.klo_n * one.krow_off, 0), d.k)
                Ad = A2[tm * bm:(tm + 1) * bm].copy()
                Ad[:, k_lo:k_lo + 4] = 0.0
                c, _, _ = GR.reference_tiles(Ad, B[nb:nb + bn], C0[nc:nc + bn, tm * bm:(tm + 1) * bm], one, bm, bn)
                bad[nc:nc + bn, tm * bm:(tm + 1) * bm] = c
        err = np.abs((bad.astype(np.longdouble) - ref)[w]).astype(np.float64)
        assert (err > bound[w]).mean() > 0.9, d


def test_poison_sits_outside_what_the_reference_reads():
    """Every generator case: the expected result is finite although A and B carry NaN wherever the launch must not read; with the
    poison cut for 128 x 128 a smaller tile's reference is finite too."""
    for idx, d in enumerate(_grid()):
        for bm, bn in SHAPES:
            for pbm, pbn in {(bm, bn), (128, 128)}:
                p = GR.Problem(d, pbm, pbn, seed=idx)
                buf, C0, must = p.c_buffer(bm, bn)
                want, w, _ = GR.reference_tiles(p.A, p.B, C0, d, bm, bn)
                assert np.array_equal(w, must) and np.isfinite(want[must]).all(), (d, bm, bn, pbm, pbn)
                assert (np.ascontiguousarray(want[~must]).view(np.uint64) == GR.SENTINEL).all()
                p.check(_expected_buffer(p, buf, want), bm, bn)
        if d.klo_m or d.nblk_stride > 1 or (d.klo_n and d.krow_off >= 0):
            p = GR.Problem(d, 128, 128, seed=idx)
            assert np.isnan(p.A).any() or np.isnan(p.B).any(), d


def _expected_buffer(p, buf, want):
    out = buf.copy()
    out[GR.GUARD_M:GR.GUARD_M + p.d.m, GR.GUARD_N:GR.GUARD_N + p.d.c_rows] = want.T
    return out


def test_check_rejects_wrong_results():
    d = Desc(m=256, n=256, k=64, alpha=-1.0, beta=1.0, tri=1)
    p = GR.Problem(d, 64, 64, seed=5)
    buf, C0, must = p.c_buffer(64, 64)
    want, _, _ = GR.reference_tiles(p.A, p.B, C0, d, 64, 64)
    good = _expected_buffer(p, buf, want)
    p.check(good, 64, 64)
    for where in [(GR.GUARD_M + 3, GR.GUARD_N + 200), (GR.GUARD_M + 200, GR.GUARD_N + 3), (0, 0), (GR.GUARD_M, GR.GUARD_N - 1),
                  (GR.GUARD_M + 256, GR.GUARD_N)]:
        bad = good.copy()
        bad[where] += 1.0
        with pytest.raises(AssertionError):
            p.check(bad, 64, 64)
