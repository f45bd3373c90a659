"""The split-k f64 GEMM of gumbi_amd/csrc/gemm_splitk.hpp through its test door ``gmb_blk_gemm_splitk`` (C ABI 16), against the
numpy restatement of the launch semantics in tests/gemm_reference.py (operands, NaN poison, sentinels).  Needs a GPU (``-m gpu``).

* Integer operands in [-8, 8]: every partial sum of every slice in any order is an exactly representable integer (|sum| <= 64 k
  <= 2^19 at k = 4112), so the result must equal numpy's float64 product BIT FOR BIT whatever the number of slices -- a slice
  that is dropped, read twice, or read one k-row too far cannot pass; NaN sits around every operand and, with beta == 0, in C
  itself; the sentinel outside the written tiles (the skipped ``tri`` tiles included) is compared bitwise.
* Standard-normal operands with beta != 0 inside the helper's derived bound gamma_{k + 3} (|alpha| |B| |A|^T + |beta| |C0|), which
  holds for ANY summation order -- the slice sums included.
* The same bits call after call; the refused pins launch nothing and report ``slices_used == 0``.
"""
import numpy as np
import pytest

import gemm_reference as GR
from gemm_reference import Desc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(gpu):
    from gumbi_amd.engine import Engine

    with Engine(0) as e:
        yield e


def _launch(eng, p, bufC, d, slices=-1, refuse=False):
    import torch

    dev = torch.device("cuda:0")
    tA = torch.from_numpy(p.bufA).to(dev)
    tB = torch.from_numpy(p.bufB).to(dev)
    tC = torch.from_numpy(bufC).to(dev)
    torch.cuda.synchronize()  # the copies run on torch's stream, the product on the engine's own
    args = (tC.data_ptr() + 8 * p.offC, p.ldc, tA.data_ptr() + 8 * p.offA, p.lda, tB.data_ptr() + 8 * p.offB, p.ldb, d.m, d.n, d.k,
            d.alpha, d.beta, d.tri, slices)
    used = None
    try:
        if refuse:
            with pytest.raises(ValueError):
                eng.blk_gemm_splitk(*args)
            used = eng.splitk_slices_used
        else:
            used = eng.blk_gemm_splitk(*args)
    finally:
        torch.cuda.synchronize()
    return tC.cpu().numpy(), used


def run(eng, d, slices=-1, kind="exact", seed=0):
    p = GR.Problem(d, 128, 128, kind=kind, seed=seed)
    bufC, _, must = p.c_buffer(128, 128)
    got, used = _launch(eng, p, bufC, d, slices)
    what = f"{d} slices={slices} -> {used} {kind}"
    assert used >= 1 and (slices < 1 or used == slices), what
    try:
        p.check(got, 128, 128, kind=kind)
    except AssertionError as exc:
        raise AssertionError(f"{what}: {exc}") from None
    return got, used


def test_one_tile_shortest_contraction(eng):
    """m = n = 128, k = 16: one k-tile, the degenerate shape -- by the rule (which must give one slice) and pinned to 1."""
    for alpha, beta in [(1.0, 0.0), (-1.0, 1.0)]:
        d = Desc(m=128, n=128, k=16, alpha=alpha, beta=beta)
        _, used = run(eng, d, slices=-1, seed=3)
        assert used == 1
        run(eng, d, slices=1, seed=3)


def test_slices_agree_on_a_long_contraction(eng):
    """k = 4112 = 16 x 257 pinned to 1, 2 and 7 slices (7: six slices of 592 and a ragged last one of 560): each exact, so all equal;
    the rule's own choice as well (more than one slice on this shape)."""
    results = []
    for alpha, beta in [(2.0, 0.0), (-1.0, 1.0)]:
        d = Desc(m=128, n=128, k=4112, alpha=alpha, beta=beta)
        per = [run(eng, d, slices=s, seed=11)[0] for s in (1, 2, 7)]
        assert np.array_equal(per[0].view(np.uint64), per[1].view(np.uint64))
        assert np.array_equal(per[0].view(np.uint64), per[2].view(np.uint64))
        got, used = run(eng, d, slices=-1, seed=11)
        assert used > 1, "the rule must split a one-tile product of k = 4112"
        assert np.array_equal(per[0].view(np.uint64), got.view(np.uint64))
        results.append(used)
    assert results[0] == results[1], "the split depends on (tiles, k) alone"


def test_triangular_update_shape(eng):
    """The corner update's form: m = 256, n = 384, tri, k = 2048, alpha = -1, beta = 1 -- five tiles, the one above the diagonal
    keeps the sentinel."""
    d = Desc(m=256, n=384, k=2048, alpha=-1.0, beta=1.0, tri=1)
    for s in (-1, 1, 3):
        run(eng, d, slices=s, seed=5)
    run(eng, Desc(m=384, n=256, k=512, alpha=-1.0, beta=1.0, tri=1), seed=6)  # more m-tiles than n-tiles: the last m-tile has none
    run(eng, Desc(m=256, n=256, k=1024, alpha=0.5, beta=0.0, tri=0), seed=7)   # rectangular, C never read


def test_real_operands_within_the_rounding_bound(eng):
    run(eng, Desc(m=128, n=128, k=4112, alpha=-1.0, beta=1.0), slices=7, kind="real", seed=21)
    run(eng, Desc(m=256, n=384, k=2048, alpha=-1.0, beta=1.0, tri=1), kind="real", seed=22)
    run(eng, Desc(m=128, n=256, k=1040, alpha=0.5, beta=-1.0), kind="real", seed=23)


def test_same_bits_call_after_call(eng):
    d = Desc(m=256, n=384, k=2048, alpha=-1.0, beta=1.0, tri=1)
    a, ua = run(eng, d, kind="real", seed=31)
    b, ub = run(eng, d, kind="real", seed=31)
    assert ua == ub
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_refused_pins_launch_nothing(eng):
    for d, s in [(Desc(m=128, n=128, k=16), 2),          # the second slice would be empty
                 (Desc(m=128, n=128, k=4112), 257),      # 257 units of 16 in 257 slices is fine ...
                 (Desc(m=128, n=128, k=4112), 258),      # ... 258 is not
                 (Desc(m=128, n=128, k=4112), 200),      # ceil(257 / 200) = 2 units per slice: slices 129 .. 199 would be empty
                 (Desc(m=128, n=128, k=64), 0),          # neither the rule nor a pin
                 (Desc(m=128, n=128, k=64), -2)]:
        p = GR.Problem(d, 128, 128, seed=1)
        bufC = p.c_buffer(128, 128)[0]
        if (d.k, s) == (4112, 257):
            got, used = _launch(eng, p, bufC, d, s)
            assert used == 257
            continue
        got, used = _launch(eng, p, bufC, d, s, refuse=True)
        assert used == 0, (d, s, used)
        assert np.array_equal(got.view(np.uint64), bufC.view(np.uint64)), "a refused launch wrote to C"
    # bad sizes
    p = GR.Problem(Desc(m=128, n=128, k=64), 128, 128, seed=1)
    bufC = p.c_buffer(128, 128)[0]
    for bad in (Desc(m=64, n=128, k=64), Desc(m=128, n=128, k=24), Desc(m=128, n=0, k=64)):
        got, used = _launch(eng, p, bufC, bad, -1, refuse=True)
        assert used == 0
        assert np.array_equal(got.view(np.uint64), bufC.view(np.uint64))
