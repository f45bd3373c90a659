"""Every f64 GEMM kernel form of gumbi_amd/csrc/gemm_f64.hpp, one launch at a time through the test door ``gmb_blk_gemm_ex``
(C ABI 13), against the numpy restatement of the launch semantics in tests/gemm_reference.py.  Needs a GPU (``-m gpu``).

Kernel forms: the LDS-DMA 128 x 128 kernel, the register-staged 128 x 128 kernel, the 64 x 64, 128 x 64 and 128 x 32 kernels each
with and without the C-prefetching (PFC) instantiation -- the out-of-place forms -- and the in-place form (C is B) on the
128 x 128, 128 x 64 and 128 x 32 tiles.  Every case pins the form and asserts that ``launched`` names it.

* Exact inputs (integers in [-8, 8], alpha, beta in {1, -1, 2, 0.5, 0}, k <= 4096): every partial sum in any order is exactly
  representable, so the result must equal numpy's float64 product BIT FOR BIT; a loop that drops, duplicates or over-reads one
  k-slice cannot pass.  One case per form and group also runs standard-normal inputs against a long-double reference inside
  the derived bound gamma_{k_eff + 3} (|alpha| |B| |A|^T + |beta| |C0|).
* Poison: everything the launch has no business reading is NaN (structural zeros of triangular operands, rows between strided
  blocks, >= 128 rows / 16 k-rows of guard around every operand); everything it has no business writing holds a sentinel bit
  pattern that is compared bitwise (skipped ``tri`` tiles, rows between strided blocks, guard bands).  With beta == 0, C is NaN
  where it must be written: the kernels must not read it.
* The PFC instantiations exist for beta != 0 only: for them the (alpha, beta) = (2, 0) cell of the scalar grid asserts that the
  door refuses the combination and launches nothing.

``gemm_f64_batched_kernel`` is the same ``gemm_f64_body`` as the non-PFC instantiations and reads the same ``GemmArgs``; it has no
door of its own and is covered by these tests through the shared body (its launch plan is checked by the gradient tests).
``gemm_f64_dma_chol_update_kernel`` is ``gemm_f64_dma_body`` under a second name.
"""
import time
from dataclasses import replace

import numpy as np
import pytest

import gemm_reference as GR
from gemm_reference import Desc
from gumbi_amd.engine import GEMM_TILE_SHAPES as SHAPES  # (BM, BN) of variant 0 .. 3

pytestmark = pytest.mark.gpu

#: name -> (variant, staging, pfc)
FORMS = {
    "dma128": (0, 1, 0), "reg128": (0, 0, 0),
    "t64x64": (1, -1, 0), "t64x64_pfc": (1, -1, 1),
    "t128x64": (2, -1, 0), "t128x64_pfc": (2, -1, 1),
    "t128x32": (3, -1, 0), "t128x32_pfc": (3, -1, 1),
}
#: (2 + 3 x 2 distinct out-of-place instantiations; the DMA body's second kernel name, the Cholesky's bulk update, is the same code)
ALL = sorted(FORMS)


@pytest.fixture(scope="module")
def eng(gpu):
    from gumbi_amd.engine import Engine

    t0 = time.time()
    with Engine(0) as e:
        yield e
    print(f"\n[test_gpu_gemm] module wall time {time.time() - t0:.1f} s")


def _launch(eng, p, bufC, d, variant=-1, staging=-1, pfc=-1, order=-1, strip=-1, refuse=False):
    """Upload, launch, download.  Returns (C buffer after the launch, launched); ``refuse``: the door must answer GMB_EINVAL
    (ValueError) -- launched is None then."""
    import torch

    dev = torch.device("cuda:0")
    tA = torch.from_numpy(p.bufA).to(dev)
    tB = torch.from_numpy(p.bufB).to(dev)
    tC = tB if p.in_place else torch.from_numpy(bufC).to(dev)
    torch.cuda.synchronize()  # the copies run on torch's stream, the product on the engine's own
    args = (tC.data_ptr() + 8 * p.offC, tA.data_ptr() + 8 * p.offA, tB.data_ptr() + 8 * p.offB, p.ldc, p.lda, p.ldb, d.m, d.n,
            d.k, d.alpha, d.beta, d.tri, d.tri_off, d.nblk_stride, d.cblk_stride, d.klo_m, d.klo_n, d.khi_n, d.krow_off,
            d.krow_stride, variant, staging, pfc, order, strip)
    launched = None
    try:
        if refuse:
            with pytest.raises(ValueError):
                eng.blk_gemm_ex(*args)
        else:
            launched = eng.blk_gemm_ex(*args)
    finally:
        torch.cuda.synchronize()
    return tC.cpu().numpy(), launched


def run(eng, form, d, kind="exact", seed=0, order=-1, strip=-1, pfc=None, tag=""):
    variant, staging, fpfc = FORMS[form]
    pfc = fpfc if pfc is None else pfc
    bm, bn = SHAPES[variant]
    p = GR.Problem(d, bm, bn, kind=kind, seed=seed)
    bufC, _, must = p.c_buffer(bm, bn)
    got, launched = _launch(eng, p, bufC, d, variant, staging, pfc, order, strip)
    what = f"{form} {tag} {d} order={order} strip={strip} pfc={pfc} {kind}"
    assert launched["variant"] == variant and launched["in_place"] == 0 and launched["pfc"] == pfc, (what, launched)
    assert launched["dma"] == (1 if staging == 1 else 0), (what, launched)
    if order >= 0:
        assert launched["order"] == order, (what, launched)
    if strip >= 0:
        assert launched["strip"] == strip, (what, launched)
    assert launched["grid"] >= int(must.sum()) // (bm * bn) > 0, (what, launched)  # at least one block per tile to write
    try:
        p.check(got, bm, bn, kind=kind)
    except AssertionError as exc:
        raise AssertionError(f"{what}: {exc}") from None
    return launched


def refused(eng, d, variant, staging=-1, pfc=-1, order=-1, strip=-1, in_place=False):
    """The door must answer GMB_EINVAL and launch nothing: C keeps every bit."""
    bm, bn = SHAPES[variant if 0 <= variant <= 3 else 0]
    p = GR.Problem(d, bm, bn, seed=1, in_place=in_place)
    bufC = p.bufB if in_place else p.c_buffer(bm, bn)[0]
    got, _ = _launch(eng, p, bufC, d, variant, staging, pfc, order, strip, refuse=True)
    assert np.array_equal(got.view(np.uint64), bufC.view(np.uint64)), "a refused launch wrote to C"


# ---- layouts and scalars ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ALL)
def test_layouts_and_scalars(eng, form):
    first = True
    for (m, n) in [(128, 128), (256, 384), (384, 256)]:
        for alpha, beta in [(-1.0, 1.0), (2.0, 0.0), (0.5, -1.0), (1.0, 0.5)]:
            d = Desc(m=m, n=n, k=160, alpha=alpha, beta=beta)
            if FORMS[form][2] == 1 and beta == 0.0:  # no such launch exists: the door says so
                refused(eng, d, FORMS[form][0], pfc=1)
                continue
            run(eng, form, d, seed=m + n)
            if first:
                run(eng, form, d, kind="real", seed=1)
                first = False


# ---- contraction-length edges -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ALL)
def test_contraction_length_edges(eng, form):
    """k = 16 .. 144: 2, 4, 6, 8, 10, 16, 18 stages of the DMA ring of four (fewer than, equal to, more than the ring; the "stay
    on the last tile" branch), and 1 .. 9 k-tiles of the register loop (odd and even counts around its peeled last tile)."""
    for k in (16, 32, 48, 64, 80, 128, 144):
        for alpha, beta in [(-1.0, 1.0)] + ([(2.0, 0.0)] if FORMS[form][2] == 0 else [(1.0, 0.5)]):
            run(eng, form, Desc(m=256, n=128, k=k, alpha=alpha, beta=beta), seed=k)
    run(eng, form, Desc(m=128, n=256, k=80, alpha=0.5, beta=-1.0), kind="real", seed=2)


@pytest.mark.parametrize("form", ALL)
@pytest.mark.parametrize("k", [1024, 1040])
def test_pfc_rule_boundary(eng, form, k):
    """k = 1024 / 1040 straddle the launcher's PFC rule (k <= 1024); the prefetch is pinned on and off at both."""
    d = Desc(m=128, n=256, k=k, alpha=-1.0, beta=1.0)
    run(eng, form, d, seed=k)
    if FORMS[form][0] != 0:
        run(eng, form, d, seed=k + 1, pfc=1 - FORMS[form][2])
    if k == 1040:
        run(eng, form, replace(d, m=128, n=128), kind="real", seed=4)


def test_pfc_by_the_rule(eng):
    """pfc = -1: the launcher's own rule -- beta != 0 and k <= 1024 and out of place."""
    for k, beta, want in [(1024, 1.0, 1), (1040, 1.0, 0), (1024, 0.0, 0)]:
        d = Desc(m=128, n=128, k=k, alpha=1.0, beta=beta)
        p = GR.Problem(d, 64, 64, seed=k)
        bufC = p.c_buffer(64, 64)[0]
        got, launched = _launch(eng, p, bufC, d, variant=1)
        assert launched["pfc"] == want and launched["variant"] == 1, launched
        p.check(got, 64, 64)


# ---- tri --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ALL)
def test_tri(eng, form):
    """The set of written tiles equals the rule's set exactly (sentinel bits everywhere else), m > n and n > m."""
    bm, bn = SHAPES[FORMS[form][0]]
    offs = [0, 128, -128] + ([64, -64] if bn <= 64 else [])  # +-64 moves the rule by a whole tile only where BN divides 64
    first = True
    for m, n in [(512, 256), (256, 512)]:
        for off in offs:
            for alpha, beta in [(-1.0, 1.0)] + ([(2.0, 0.0)] if FORMS[form][2] == 0 else []):
                d = Desc(m=m, n=n, k=48, alpha=alpha, beta=beta, tri=1, tri_off=off)
                run(eng, form, d, seed=off + m)
                if first:
                    run(eng, form, d, kind="real", seed=5)
                    first = False


# ---- k ranges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ALL)
def test_k_ranges(eng, form):
    s = 640  # five block rows: not a power of two
    b0 = 0.0 if FORMS[form][2] == 0 else 0.5
    base = Desc(m=s, n=s, k=s, alpha=-1.0, beta=1.0)
    cases = [
        replace(base, klo_n=1), replace(base, khi_n=1), replace(base, klo_m=1),
        replace(base, klo_n=1, khi_n=1),                       # every tile contracts its own block only
        replace(base, klo_n=1, alpha=2.0, beta=b0), replace(base, khi_n=1, alpha=2.0, beta=b0),
        replace(base, m=s, n=256, k=384, klo_m=1),             # tm * BM >= k for the last m-tiles: C = beta * C exactly
        replace(base, m=s, n=256, k=384, klo_m=1, alpha=1.0, beta=b0),   # ... and zeros for beta = 0
        replace(base, klo_n=1, krow_off=128), replace(base, klo_n=1, krow_off=-128),
        replace(base, khi_n=1, krow_off=128), replace(base, khi_n=1, krow_off=-128),   # k_hi <= 0 for the first tile(s)
        replace(base, khi_n=1, krow_off=-128, alpha=1.0, beta=b0),
        replace(base, klo_n=1, khi_n=1, krow_off=-128),
        replace(base, n=256, klo_n=1, krow_stride=2), replace(base, n=256, khi_n=1, krow_stride=3),
        replace(base, n=256, klo_n=1, khi_n=1, krow_stride=2, krow_off=128),
        replace(base, klo_m=1, klo_n=1),
    ]
    for i, d in enumerate(cases):
        run(eng, form, d, seed=i, tag=f"case {i}")
    run(eng, form, cases[3], kind="real", seed=6)
    run(eng, form, replace(cases[0], m=256, n=256, k=256), kind="real", seed=7)


# ---- strides ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ALL)
def test_strides(eng, form):
    b0 = 0.0 if FORMS[form][2] == 0 else 1.0
    cases = []
    for st in (2, 3):
        for cb in (0, 1):
            cases.append(Desc(m=256, n=384, k=64, alpha=-1.0, beta=1.0, nblk_stride=st, cblk_stride=cb))
            cases.append(Desc(m=640, n=256, k=64, alpha=-1.0, beta=1.0, nblk_stride=st, cblk_stride=cb, tri=1, tri_off=128))
            cases.append(Desc(m=256, n=256, k=640, alpha=1.0, beta=b0, nblk_stride=1, cblk_stride=cb, klo_n=1, krow_off=128, krow_stride=st))
            # rows `st` blocks apart in memory that stand for every (5 - st)-th block row: R(tn) and noff(tn) part ways
            cases.append(Desc(m=256, n=256, k=640, alpha=1.0, beta=b0, nblk_stride=st, cblk_stride=cb, klo_n=1, krow_off=128,
                              krow_stride=5 - st))
            cases.append(Desc(m=256, n=256, k=640, alpha=-1.0, beta=1.0, nblk_stride=st, cblk_stride=cb, klo_n=1, khi_n=1, krow_off=128,
                              krow_stride=5 - st))
            cases.append(Desc(m=256, n=256, k=640, alpha=-1.0, beta=1.0, nblk_stride=st, cblk_stride=cb, klo_n=1, krow_off=128))
    # grad_sigma_inv_rows(shard = 1, nshards = 2, packed) at Np = 640: block rows 1, 3 of Sigma^-1 = U U^T out of the full-size factor
    cases.append(Desc(m=640, n=256, k=640, alpha=1.0, beta=0.0 if FORMS[form][2] == 0 else 1.0, klo_n=1, krow_off=128, tri=1, tri_off=128,
                      nblk_stride=2, cblk_stride=1))
    # ... and unpacked (rows at their global position)
    cases.append(Desc(m=640, n=256, k=640, alpha=1.0, beta=0.0 if FORMS[form][2] == 0 else 1.0, klo_n=1, krow_off=128, tri=1, tri_off=128,
                      nblk_stride=2, cblk_stride=0))
    # the capacity driver's Sigma^-1 accumulation: G = 3, first = 1, chunk [k0, k1) = [0, 4): rows 1, 4 (row 4 starts past the chunk)
    cases.append(Desc(m=512, n=256, k=512, alpha=1.0, beta=1.0, klo_n=1, krow_off=128, tri=1, tri_off=128, nblk_stride=3, cblk_stride=1))
    # the drivers' update of a rank's packed rows of U: contiguous rows that stand for every G-th block row (G = 2, first = 1)
    cases.append(Desc(m=256, n=256, k=512, alpha=-1.0, beta=1.0, klo_n=1, krow_stride=2, krow_off=128))
    # the capacity driver's trailing update: strided rows of the panel into packed owned rows
    cases.append(Desc(m=384, n=256, k=128, alpha=-1.0, beta=1.0, tri=1, tri_off=128, nblk_stride=3, cblk_stride=1))
    for i, d in enumerate(cases):
        run(eng, form, d, seed=i, tag=f"case {i}")
    run(eng, form, cases[-4], kind="real", seed=8)


# ---- orders -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ALL)
def test_orders_and_strips(eng, form):
    b0 = 0.0 if FORMS[form][2] == 0 else 1.0
    s = 640
    for order, f in [(1, dict(klo_n=1)), (2, dict(khi_n=1))]:
        run(eng, form, Desc(m=s, n=s, k=s, alpha=-1.0, beta=1.0, **f), order=order, seed=order)
        run(eng, form, Desc(m=s, n=s, k=s, alpha=1.0, beta=b0, tri=1, **f), order=order, seed=order + 2)
        run(eng, form, Desc(m=384, n=s, k=s, alpha=1.0, beta=1.0, tri=1, tri_off=128, **f), order=order, seed=order + 4)
        run(eng, form, Desc(m=s, n=s, k=s, alpha=-1.0, beta=1.0, **f), order=0, strip=0, seed=order + 6)
    run(eng, form, Desc(m=s, n=s, k=s, alpha=-1.0, beta=1.0, klo_n=1), order=1, kind="real", seed=9)
    for tri in (0, 1):
        for strip in (8, 0, 3):
            run(eng, form, Desc(m=2560, n=384, k=32, alpha=-1.0, beta=1.0, tri=tri), order=0, strip=strip, seed=tri)
        run(eng, form, Desc(m=2560, n=384, k=32, alpha=2.0, beta=b0, tri=tri, tri_off=-128, nblk_stride=2), order=0, strip=8, seed=tri + 2)


@pytest.mark.parametrize("form", ALL)
def test_many_tiles(eng, form):
    """24 x 24 blocks of 128 at k = 32 (75 MB of C): every XCD run and several rounds of workgroup slots."""
    launched = run(eng, form, Desc(m=3072, n=3072, k=32, alpha=-1.0, beta=1.0), order=0, strip=8, seed=11)
    bm, bn = SHAPES[FORMS[form][0]]
    assert launched["grid"] >= 3072 // bm * (3072 // bn)
    run(eng, form, Desc(m=3072, n=3072, k=32, alpha=-1.0, beta=1.0, tri=1), order=0, strip=0, seed=12)


# ---- in place ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 2, 3])
@pytest.mark.parametrize("n", [128, 384, 1152])
def test_in_place(eng, variant, n):
    """C is B (the panel / predict triangular solves): m = k = 128, alpha = 1, beta = 0, ldb > n.  Exact result, guard rows and
    guard k-rows untouched, A between NaN guard columns."""
    d = Desc(m=128, n=n, k=128, alpha=1.0, beta=0.0)
    p = GR.Problem(d, 128, 128, seed=n + variant, in_place=True)
    got, launched = _launch(eng, p, None, d, variant=variant)
    assert launched["variant"] == variant and launched["in_place"] == 1 and launched["pfc"] == 0 and launched["dma"] == 0, launched
    assert launched["strip"] == 0 and launched["grid"] >= n // SHAPES[variant][1], launched
    p.check_in_place(got)


# ---- the launcher's own choice ----------------------------------------------------------------------------------------------
def _model_variant(nact, slots):
    """launch_gemm's documented model: T tiles on S workgroup slots take max(1, T / S + 1/2) tile times; intrinsic rates 73 / 63 /
    65 TF/s for 128 x 128, 64 x 64, 128 x 64; 128 x 64 is tried first, then 64 x 64, each taken when it scores higher."""
    rate, per = {0: 73.0, 1: 63.0, 2: 65.0}, {0: 1, 1: 4, 2: 2}
    score = lambda v: rate[v] * per[v] / max(1.0, nact * per[v] / slots + 0.5)  # noqa: E731
    v = 0
    if score(2) > score(v):
        v = 2
    if score(1) > score(v):
        v = 1
    return v


def test_model_choice(eng):
    """variant = -1 at three sizes: ``launched`` names the tile shape the documented model predicts (64 x 64 for one tile and for
    a launch of less than a round, 128 x 128 with LDS-DMA staging once the launch is several rounds long) and the result is exact.
    Poison at 128 granularity: safe for whichever shape runs."""
    import torch

    slots = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    seen = set()
    for m, n, k in [(128, 128, 64), (1024, 1536, 32), (4608, 4608, 16)]:
        d = Desc(m=m, n=n, k=k, alpha=-1.0, beta=1.0, tri=1 if m == 1024 else 0)
        nact = sum(1 for tm in range(m // 128) for tn in range(n // 128) if not d.tri or tn * 128 + 127 >= tm * 128)
        want = _model_variant(nact, slots)
        seen.add(want)
        bm, bn = SHAPES[want]
        p = GR.Problem(d, 128, 128, seed=m)
        bufC = p.c_buffer(bm, bn)[0]
        got, launched = _launch(eng, p, bufC, d)
        assert launched["variant"] == want, (m, n, nact, slots, launched)
        assert launched["dma"] == (1 if want == 0 else 0) and launched["pfc"] == (1 if want != 0 else 0), launched
        assert launched["order"] == 0 and launched["strip"] == (8 if m // bm >= 2 else 0), launched
        p.check(got, bm, bn)
    assert seen == {0, 1}, (seen, slots)


# ---- what the door must refuse ----------------------------------------------------------------------------------------------
def test_door_refuses_what_the_launcher_cannot_produce(eng):
    base = Desc(m=256, n=256, k=256, alpha=-1.0, beta=1.0)
    refused(eng, replace(base, beta=0.0), variant=1, pfc=1)                    # PFC with beta == 0
    refused(eng, base, variant=0, pfc=1)                                       # no PFC instantiation of the 128 x 128 tile
    for v in (1, 2, 3):
        refused(eng, base, variant=v, staging=1)                               # DMA staging on a small tile
    refused(eng, replace(base, klo_n=1, nblk_stride=2), variant=0, order=1)    # n-major orders need contiguous rows
    refused(eng, replace(base, klo_n=1, tri=1, tri_off=-128), variant=0, order=1)   # ... and tri_off >= 0
    refused(eng, replace(base, khi_n=1), variant=0, order=1)                   # order 1 is the klo_n order
    refused(eng, replace(base, klo_n=1), variant=0, order=2)
    refused(eng, base, variant=0, order=1)                                     # no triangular operand
    refused(eng, replace(base, klo_n=1, khi_n=1), variant=0, order=1)
    refused(eng, replace(base, klo_n=1, klo_m=1), variant=0, order=1)
    refused(eng, replace(base, klo_n=1), variant=0, order=1, strip=8)          # strips belong to order 0
    refused(eng, replace(base, klo_m=1), variant=0, strip=8)
    refused(eng, replace(base, m=128), variant=0, strip=8)                     # one m-tile: nothing to rasterise
    refused(eng, base, variant=4)
    inp = Desc(m=128, n=256, k=128, alpha=1.0, beta=0.0)
    refused(eng, replace(inp, m=256, k=256), variant=0, in_place=True)         # in place with m != 128
    refused(eng, inp, variant=1, in_place=True)                                # ... on the 64 x 64 tile
    refused(eng, inp, variant=0, staging=1, in_place=True)
    refused(eng, replace(inp, beta=1.0), variant=2, pfc=1, in_place=True)
    refused(eng, inp, variant=2, strip=8, in_place=True)
