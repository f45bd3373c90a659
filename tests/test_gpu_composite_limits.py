"""Composite models at the engine's structural limits, parameter by parameter -- runs on the MI355X box only.

The engine takes 16 continuous dims, 8 linear dims, 4 coregion tables plus the output table, 32 levels per table and a
noise table per output.  The structures of tests/composite_reference.py (CASES) are the smallest at which each path behind
those limits is reached: the per-wave GLOBAL copies of a table's accumulators from 9 levels on (csrc/gradient.hpp:
grad_tile_body, ``a.big``; engine.hip: grad_reduce's dgbig, its second grad_sum_partials_kernel launch, no merged landing),
small and big tables in one launch, every g_c slot, grad_diag_kernel's 32-level noise table, the largest dynamic LDS request
(grad_lds_bytes(16, 8, 5), ~50 KB), one pass per term of an additive model with a big table, a table of one diagonal tile.

The gradient is compared COMPONENT BY COMPONENT with the longdouble reference (composite_reference.grad_reference):

    |g_p - ref_p| <= K max(e64_p, floor_p)         for every p,

e64_p the float64 host path's error on the same component, floor_p = 4 eps A_p with A_p = sum_ij |M_ij dSigma_p,ij| (raised
to the host's relative error in the sigma / noise-table blocks: composite_reference.gradient_floor).  On the largest model the
components span six orders of magnitude; under a max-norm bar a table partial or a c_k that is 100 % wrong passes.  K follows
the rule of tests/test_gpu_conditioning.py: K = max(2.5 r, 1) with r the worst ratio this engine measured on an MI355X, per
case, route and parameter block, in tests/golden/composite_limits_ratios.json (made by make_composite_limits_ratios.py from
the ``RATIO <case> <route> <block> <value>`` lines every comparison prints); a comparison without a record fails.  The ratios
are measured against the longdouble reference, never against the engine.

Two launch shapes of grad_tile_kernel need sizes where longdouble is not affordable (LARGE_CASES: more than 512 direct-loop
tiles, gsplit == 1; more than 1536, per == 2 with runs that cross block rows): those are held to the float64 oracle's stored
NLML and gradient at the parity tests' bars and per parameter block.
"""
import json
from pathlib import Path

import numpy as np
import pytest

import composite_reference as CR
from oracle import gp_oracle as O
from test_gpu_parity import make_engine, rel

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
RECORD_FILE = GOLDEN / "composite_limits_ratios.json"
RECORD = json.loads(RECORD_FILE.read_text())["ratio"] if RECORD_FILE.exists() else {}
K_OF_RECORD = 2.5
EPS = np.finfo(float).eps
CASES = list(CR.CASES)


def routes(eng, theta):
    """(name, call) of every way to the gradient: gmb_factorize + gmb_nlml(grad), and gmb_evaluate with the gradient's inverse
    as a tree of launches and fused into the factorisation's launch"""
    def nlml():
        eng.set_grad_scheme(eng.GRAD_BY_SIZE)
        eng.set_theta(theta)
        eng.factorize()
        return eng.nlml(grad=True)

    def tree():
        eng.set_grad_scheme(eng.GRAD_LAUNCH_TREE)
        return eng.evaluate(theta)

    def fused():
        eng.set_grad_scheme(eng.GRAD_FUSED)
        return eng.evaluate(theta)

    return (("nlml", nlml), ("tree", tree), ("fused", fused))


# ----------------------------------------------------------------------------------------------
# covariance, entry by entry
# ----------------------------------------------------------------------------------------------
def covariance_scale(spec, theta, X):
    """sum over the terms of max |prod_t B_t| * (eta^2 + tau max |a.a'|): the size of the largest product an entry is made of"""
    blocks, terms, tables = CR.layout(spec)
    n_lin = len(spec["idx_lin"])
    G = []
    for col, L, w0, k0 in tables:
        W = theta[w0:w0 + 2 * L].reshape(L, 2)
        c = X[:, col].astype(int)
        G.append((W @ W.T + np.diag(theta[k0:k0 + L]))[c[:, None], c[None, :]])
    total = 0.0
    for tr in terms:
        F = np.ones((len(X), len(X)))
        for t in tr["tables"]:
            F = F * G[t]
        base = theta[tr["eta"]] ** 2
        if n_lin:
            A = X[:, spec["idx_lin"]] - theta[tr["c"]:tr["c"] + n_lin]
            base += theta[tr["tau"]] * np.max(np.abs(A @ A.T))
        total += np.max(np.abs(F)) * base
    return total


@pytest.mark.parametrize("case", CASES)
def test_covariance_build_matches_oracle_entrywise(gpu, case):
    """gmb_blk_covariance against O.sigma_matrix(dist_mode="direct"): lower triangle, y row, identity padding.

    Composite terms (a linear part or a table) and the kinked kinds take the direct form on EVERY tile, and the smooth plain
    kinds do on every tile of a table of three block columns that holds a diagonal entry or is ragged, so no expansion term
    applies: the bar is that of test_gpu_parity.py's diagonal tiles, 8 eps per unit of the entry's scale.  There the entry is
    eta^2 k with k <= 1 (scale eta^2); here it is (eta^2 k + tau a.a') prod_t B_t[c, c'], a sum over the terms of an additive
    model: the distance, sqrt and exp chain is the same, the linear part adds a dot product of at most 8 terms to a base of
    size <= eta^2 + tau max|a.a'|, and every table multiplies by an entry of size <= max|prod B| with one rounding each --
    so 8 eps x max|prod_t B_t| x (eta^2 + tau max|a.a'|), summed over the terms."""
    import torch

    ref = CR.reference(case)
    spec, theta, X, y = ref["spec"], ref["theta"], ref["X"], ref["y"]
    N = len(y)
    eng = make_engine(spec, theta, X, y)
    Nr, Np = (N + 1 + 127) // 128 * 128, (N + 127) // 128 * 128
    out = torch.full((Np, Nr), float("nan"), dtype=torch.float64, device="cuda:0")  # column-major Nr x Np
    torch.cuda.synchronize()
    eng.blk_covariance(out.data_ptr(), Nr)
    S = out.cpu().numpy().T
    eng.close()
    S_dir = O.sigma_matrix(spec, theta, X, dist_mode="direct")
    low = np.tril(np.ones((N, N), bool))
    scale = covariance_scale(spec, theta, X)
    err = np.max(np.abs(S[:N, :N][low] - S_dir[low]))
    print(f"COV {case}: max |S - S_oracle| = {err:.3e} = {err / (EPS * scale):.2f} eps x scale {scale:.3g}")
    assert err < 8 * EPS * scale
    assert np.array_equal(S[N, :N], y)
    assert np.array_equal(S[N + 1:, :N], np.zeros((Nr - N - 1, N)))
    pad = S[N:, N:Np]
    assert np.array_equal(np.tril(pad), np.tril(np.eye(Nr - N, Np - N)))


# ----------------------------------------------------------------------------------------------
# gradient, component by component
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_gradient_component_by_component(gpu, case):
    """Every route to the gradient against the longdouble reference under the per-component bar (module docstring); the NLML
    against the longdouble one at the parity tests' 1e-10; a second evaluation by the same route returns the same bits (the
    atomics go into per-wave copies, no two waves share one: gradient.hpp).  The old max-norm figure is printed beside the
    ratios (MAXNORM): what the per-component bar catches leaves it far below its 1e-8."""
    ref = CR.reference(case)
    spec, theta = ref["spec"], ref["theta"]
    bound = np.maximum(ref["e64"], ref["floor"])
    names = CR.block_of(spec)
    eng = make_engine(spec, theta, ref["X"], ref["y"])
    bad = []
    for route, call in routes(eng, theta):
        val, g = call()
        val2, g2 = call()
        if not (np.float64(val2).tobytes() == np.float64(val).tobytes() and g2.tobytes() == g.tobytes()):
            bad.append(f"{route}: the second evaluation differs, max |dg| = {np.max(np.abs(g2 - g)):.3e}")
        if not abs(val - ref["nlml"]) <= 1e-10 * abs(ref["nlml"]):
            bad.append(f"{route}: nlml {val!r} against {ref['nlml']!r}")
        err = np.abs(g - ref["g"])
        print(f"MAXNORM {case} {route} {np.max(err) / max(1.0, np.max(np.abs(ref['g']))):.3e}")
        assert np.max(err) < 1e-8 * max(1.0, np.max(np.abs(ref["g"])))  # (the bar of the other parity tests)
        for block, r in CR.worst_by_block(spec, err / bound).items():
            print(f"RATIO {case} {route} {block} {r:.4g}")
            rec = RECORD.get(case, {}).get(route, {}).get(block)
            if rec is None:
                bad.append(f"{route} {block}: no recorded ratio (measured {r:.3g})")
            elif not r <= max(K_OF_RECORD * rec, 1.0):
                p = max((i for i, n in enumerate(names) if n == block), key=lambda i: err[i] / bound[i])
                bad.append(f"{route} {block}: theta[{p}] off by {err[p]:.3e} = {r:.3g} x max(e64 {ref['e64'][p]:.2e}, floor "
                           f"{ref['floor'][p]:.2e}), recorded {rec:.3g}; g_p = {ref['g'][p]:.3e}")
    eng.close()
    assert not bad, f"{case}: " + "; ".join(bad)


# ----------------------------------------------------------------------------------------------
# prediction at every level of every table
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_prediction_at_every_level(gpu, case):
    """Mean within 1e-8 relative and variance within 1e-9 absolute of O.predict(dist_mode="direct"), with and without noise,
    at test points that take every level of every table: by the triangular solve behind gmb_factorize, and as one GEMM
    against the inverse factor the fused evaluation leaves."""
    ref = CR.reference(case)
    spec, theta, X, y, Xs = (ref[k] for k in ("spec", "theta", "X", "y", "Xs"))
    want = {wn: O.predict(spec, theta, X, y, Xs, with_noise=wn, dist_mode="direct") for wn in (True, False)}
    eng = make_engine(spec, theta, X, y)
    eng.factorize()
    for form in (0, 1):
        if form:
            eng.set_grad_scheme(eng.GRAD_FUSED)
            eng.evaluate(theta)
        for wn in (True, False):
            mu, var = eng.predict(Xs, with_noise=wn)
            assert eng.timings()["predict_gemm_form"] == form
            mu_r, var_r = want[wn]
            print(f"PREDICT {case} form {form} noise {int(wn)}: mean rel {rel(mu, mu_r):.2e} var abs {np.max(np.abs(var - var_r)):.2e}")
            assert rel(mu, mu_r) < 1e-8 and np.max(np.abs(var - var_r)) < 1e-9
    eng.close()


# ----------------------------------------------------------------------------------------------
# the launch shapes of grad_tile_kernel beyond 512 and beyond 1536 direct-loop tiles
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CR.LARGE_CASES)
def test_direct_loop_launches_beyond_the_shared_tile_form(gpu, case):
    """Models that do not take the interior kernel (a kinked kind; a linear part and a table) send EVERY lower-triangle tile
    through grad_tile_kernel's direct loops.  N = 4224: 561 tiles in one launch -- more than 512, so gsplit == 1, one workgroup
    per tile (with a 9-level table: the global copies indexed by the plain blockIdx.x); N = 7040: 1540 tiles for 1536
    workgroups, per == 2, runs of two tiles that cross from one block row into the next.  Longdouble is not affordable at
    these sizes and neither is the oracle on the GPU machine: NLML and gradient of the float64 oracle are stored
    (tests/golden/make_composite_limits_goldens.py), the problem comes back from its seed.  Bars: the parity tests' (NLML 1e-10
    relative, gradient max-norm 1e-8 max(1, max|g|)), and per parameter block 1e-8 of the block's own largest component --
    a block is one parameter for the plain models."""
    gold = np.load(GOLDEN / "composite_limits_goldens.npz")
    spec, theta, X, y = CR.large_problem(case)
    assert np.array_equal(theta, gold[f"{case}/theta"])
    val_r, g_r = float(gold[f"{case}/nlml"]), gold[f"{case}/grad"]
    tiles = (len(y) + 127) // 128
    assert tiles * (tiles + 1) // 2 > (1536 if case.endswith("n7040") else 512)
    eng = make_engine(spec, theta, X, y)
    got = []
    for _ in range(2):
        got.append(eng.evaluate(theta))
    eng.factorize()
    got.append(eng.nlml(grad=True))
    eng.close()
    assert np.float64(got[0][0]).tobytes() == np.float64(got[1][0]).tobytes() and got[0][1].tobytes() == got[1][1].tobytes()
    for val, g in got[1:]:
        by_block = {}
        for name, e, r in zip(CR.block_of(spec), np.abs(g - g_r), np.abs(g_r)):
            worst = by_block.setdefault(name, [0.0, 0.0])
            worst[0], worst[1] = max(worst[0], e), max(worst[1], r)
        print(f"LARGE {case}: nlml rel {abs(val - val_r) / abs(val_r):.2e}  " + "  ".join(f"{b} {e / r:.2e}" for b, (e, r) in by_block.items()))
        assert abs(val - val_r) <= 1e-10 * abs(val_r)
        assert np.max(np.abs(g - g_r)) < 1e-8 * max(1.0, np.max(np.abs(g_r)))
        for b, (e, r) in by_block.items():
            assert e <= 1e-8 * r, (case, b, e, r)
