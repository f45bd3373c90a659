"""Pathwise posterior draws -- ``gmb_paths_prepare`` / ``gmb_paths_eval`` / ``gmb_paths_eval_own`` -- on the MI355X against the numpy
reference of tests/pathwise_reference.py (itself pinned by tests/test_pathwise_cpu.py), and ``draw_paths`` / ``propose_thompson`` on
top of them.  Needs a GPU (``-m gpu``).

Bars, each copied from where the project states it:

* all-draws and own-draw values against the reference: ``1e-8 max|ref|`` absolute (the bar for means, tests/test_gpu_joint.py);
* own-draw gradients against the reference: ``1e-8 max|ref|`` absolute (tests/test_gpu_predict_grad.py);
* own-draw values against the matching entries of ``paths_eval``: 1e-10 relative;
* the mean of an antithetic pair against ``engine.predict`` (``with_noise=False``): 1e-9 relative;
* determinism, the call forms, the state contract: bit-identical.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import abi_forms as AF
import pathwise_reference as PR
from gumbi_amd import pathwise
from oracle import gp_oracle as O
from test_gpu_abi_forms import PACKED_HOST, STRIDED_DEVICE, STRIDED_HOST, Buf, mat_in, mat_out, same_bits, sync, take, take_vec, vec_out
from test_gpu_parity import GOLD, golden_spec, make_engine, rel
from test_gpu_predict_grad import DISPATCH_DIMS, frontend_dataset, points, table

pytestmark = pytest.mark.gpu

SF = [(1, 64), (16, 256), (17, 1000), (80, 1000)]  # one draw; one accumulator tile; across a 16-seam; across a draw block -- F ragged


@functools.lru_cache(maxsize=None)
def problem(N, d, kind, S, F, ard=True, antithetic=False):
    """model, path inputs and the reference's coefficients A (N, S): computed once, shared, never written"""
    spec, theta, X, y = table(N, d, kind, ard=ard)
    inputs = pathwise.path_inputs(kind, S, F, d, N, seed=100 * S + F, antithetic=antithetic)
    A = PR.coefficients(spec, theta, X, y, *inputs)
    return spec, theta, X, y, inputs, A


def prepared(spec, theta, X, y, inputs):
    eng = make_engine(spec, theta, X, y)
    eng.factorize()
    eng.paths_prepare(*inputs)
    return eng


def check_values(got, ref, what):
    scale, err = float(np.max(np.abs(ref))), float(np.max(np.abs(got - ref)))
    print(f"{what}: max |Y - Y_ref| = {err:.3e}, max |Y_ref| = {scale:.3e}, ratio {err / scale:.2e}")
    assert got.shape == ref.shape
    assert err <= 1e-8 * scale


def check_both(N, d, kind, S, F, M, what, ard=True):
    """paths_eval and paths_eval_own (a third of the points ON training points) against the reference, and against each other"""
    spec, theta, X, y, inputs, A = problem(N, d, kind, S, F, ard)
    omega, phase, w, eps = inputs
    Xs = points(X, M, list(range(d)), on_train=M // 3)
    draw = (np.arange(M) * 7) % S
    with prepared(spec, theta, X, y, inputs) as eng:
        Y = eng.paths_eval(Xs)
        val, G = eng.paths_eval_own(Xs, draw)
    check_values(Y, PR.all_draws(spec, theta, X, Xs, omega, phase, w, A), f"{what} all draws")
    r_val, r_G = PR.own_draws(spec, theta, X, Xs, draw, omega, phase, w, A)
    check_values(val, r_val, f"{what} own values")
    check_values(G, r_G, f"{what} own gradients")
    assert np.all(np.isfinite(G[:M // 3])), "the gradient at a coincident point is finite"
    assert rel(val, Y[draw, np.arange(M)]) <= 1e-10


# ---- 1. against the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,F", SF)
@pytest.mark.parametrize("kind", O.KINDS)
def test_matches_the_reference(gpu, kind, S, F):
    check_both(300, 3, kind, S, F, 333, f"{kind} N=300 d=3 S={S} F={F} M=333")


def test_eight_block_columns_and_several_point_tiles(gpu):
    check_both(1000, 3, "Matern32", 17, 1000, 2000, "Matern32 N=1000 S=17 F=1000 M=2000")


@pytest.mark.parametrize("d", DISPATCH_DIMS)
@pytest.mark.parametrize("kind", O.KINDS)
def test_every_padded_width(gpu, kind, d):
    check_both(200, d, kind, 17, 130, 70, f"{kind} N=200 d={d} S=17 F=130 M=70")


def test_shared_lengthscale(gpu):
    check_both(300, 3, "Matern52", 16, 256, 333, "Matern52 shared lengthscale", ard=False)


def test_antithetic_pairs_average_to_predict(gpu):
    spec, theta, X, y, inputs, _ = problem(300, 3, "Matern52", 16, 256, True, True)
    Xs = points(X, 333, [0, 1, 2], on_train=111)
    with prepared(spec, theta, X, y, inputs) as eng:
        Y = eng.paths_eval(Xs)
        mu, _ = eng.predict(Xs, with_noise=False)
    pair = 0.5 * (Y[0::2] + Y[1::2])
    worst = max(rel(p, mu) for p in pair)
    print(f"mean of an antithetic pair vs predict: {worst:.2e} relative; spread of the draws {float(np.std(Y - mu)):.3f}")
    assert worst <= 1e-9 and float(np.std(Y - mu)) > 1e-3


# ---- 2. determinism, state, staleness --------------------------------------------------------------------------------------------------
def test_repeats_and_leaves_the_state(gpu):
    spec, theta, X, y, inputs, _ = problem(300, 3, "Matern52", 17, 1000)
    Xs = points(X, 333, [0, 1, 2], on_train=111)
    draw = np.arange(333) % 17

    def state(eng):
        eng.factorize()
        mu, var = eng.predict(Xs)
        jm, jc = eng.predict_joint(Xs[:40], with_noise=False, jitter=1e-6)
        eng.factorize()
        f, g = eng.nlml(grad=True)
        eng.factorize()
        return mu.tobytes(), var.tobytes(), jm.tobytes(), jc.tobytes(), np.float64(f).tobytes(), np.asarray(g).tobytes(), eng.copy_v().tobytes()

    with make_engine(spec, theta, X, y) as eng:
        before = state(eng)
        eng.paths_prepare(*inputs)
        a, b = eng.paths_eval(Xs), eng.paths_eval(Xs)
        va, vb = eng.paths_eval_own(Xs, draw), eng.paths_eval_own(Xs, draw)
        v_only = eng.paths_eval_own(Xs, draw, grad=False)
        mid = eng.predict(Xs)
        eng.paths_prepare(*inputs)
        c = eng.paths_eval(Xs)
        assert eng.factor_is_current()
        eng.paths_clear()
        with pytest.raises(ValueError, match="no paths"):
            eng.paths_eval(Xs)
        after = state(eng)
    assert a.tobytes() == b.tobytes() == c.tobytes()
    assert va[0].tobytes() == vb[0].tobytes() == v_only[0].tobytes() and va[1].tobytes() == vb[1].tobytes() and v_only[1] is None
    assert mid[0].tobytes() == before[0] and mid[1].tobytes() == before[1]
    assert before == after


def test_stale_paths_are_refused(gpu):
    from gumbi_amd.engine import GMB_EINVAL

    spec, theta, X, y, inputs, _ = problem(300, 3, "Matern52", 16, 256)
    Xs = points(X, 50, [0, 1, 2])
    with prepared(spec, theta, X, y, inputs) as eng:
        eng.paths_eval(Xs)
        eng.set_theta(theta * 1.01)
        eng.set_theta(theta)
        eng.factorize()
        rc, _, clean = raw_eval(eng, Xs)
        assert rc == GMB_EINVAL and clean, "after gmb_set_theta"
        with pytest.raises(ValueError, match="stale"):
            eng.paths_eval_own(Xs, np.zeros(50, np.int32))
        eng.paths_prepare(*inputs)
        eng.paths_eval(Xs)
        eng.append(X[:2] + 0.01, y[:2])
        rc, _, clean = raw_eval(eng, Xs)
        assert rc == GMB_EINVAL and clean, "after gmb_append"
        assert "stale" in eng._lib.gmb_last_error(eng._h).decode()


# ---- 3. refusals and call forms -------------------------------------------------------------------------------------------------------
def raw_eval(eng, Xs, form=PACKED_HOST, S=None, null=(), pad=3):
    """``gmb_paths_eval`` with guarded buffers: ``(status, Y or None, clean)`` -- ``clean``: the output still carries its fill."""
    M, D = Xs.shape
    S = int(getattr(eng, "n_paths", 0) or 1) if S is None else S
    x = mat_in(Xs, form, pad)
    out = mat_out(S, M, form, pad)
    sync()
    rc = eng._lib.gmb_paths_eval(eng._h, None if "Xs" in null else x.ptr, M, x.ld, None if "Y" in null else out.ptr, out.ld, form.memspace)
    clean = bool(np.all(np.ascontiguousarray(out.fetch()).view(np.uint64) == AF.FILL_BITS))
    if rc != 0:
        return rc, None, clean
    return rc, take(out, S, M, f"gmb_paths_eval ({form.name})"), clean


def raw_own(eng, Xs, draw, form=PACKED_HOST, grad=True, pad=3):
    M, D = Xs.shape
    x = mat_in(Xs, form, pad)
    dr = Buf(np.ascontiguousarray(draw, dtype=np.int32), form.device)
    val, g = vec_out(M, form), mat_out(M, D, form, pad)
    sync()
    rc = eng._lib.gmb_paths_eval_own(eng._h, x.ptr, M, x.ld, dr.ptr, val.ptr, g.ptr if grad else None, g.ld, form.memspace)
    clean = all(bool(np.all(np.ascontiguousarray(b.fetch()).view(np.uint64) == AF.FILL_BITS)) for b in (val, g))
    if rc != 0:
        return rc, None, clean
    what = f"gmb_paths_eval_own ({form.name})"
    return rc, (take_vec(val, M, what + " val"), take(g, M, D, what + " grad") if grad else None), clean


def raw_prepare(eng, S, F, Dc, N, null=()):
    arrays = {"omega": np.zeros((max(F, 1), Dc)), "phase": np.zeros(max(F, 1)), "w": np.ones((max(S, 1), max(F, 1))), "eps": np.ones((max(S, 1), N))}
    ptr = {k: (None if k in null else a.ctypes.data_as(C.c_void_p)) for k, a in arrays.items()}
    return eng._lib.gmb_paths_prepare(eng._h, S, F, ptr["omega"], ptr["phase"], ptr["w"], ptr["eps"])


def refuses(eng, Xs, Dc, expect, label):
    """prepare is refused with GMB_EINVAL and ``expect`` in its message; nothing is prepared, and an evaluation writes nothing"""
    from gumbi_amd.engine import GMB_EINVAL

    rc = raw_prepare(eng, 4, 16, Dc, eng.N)
    msg = eng._lib.gmb_last_error(eng._h).decode()
    assert rc == GMB_EINVAL and expect in msg, f"{label}: status {rc}, message {msg!r}"
    rc, _, clean = raw_eval(eng, Xs, S=4)
    assert rc == GMB_EINVAL and clean, f"{label}: evaluation after a refused preparation"


def test_models_outside_the_scope_are_refused(gpu):
    from test_gpu_periodic import case as periodic_case
    from test_gpu_periodic import make_engine as periodic_engine
    from test_oracle import additive_problem

    case = "composite_N140"
    spec, theta, X, y = golden_spec(case), GOLD[f"{case}/theta"], GOLD[f"{case}/X"], GOLD[f"{case}/y"]
    with make_engine(spec, theta, X, y) as eng:
        eng.factorize()
        refuses(eng, X[:5], 2, "linear dimensions", "composite golden (linear x coregion)")
    spec, theta, X, y = additive_problem(n=60, two_outputs=True, lin=False, hetero=True)
    with make_engine(spec, theta, X, y) as eng:
        eng.factorize()
        refuses(eng, X[:5], len(spec["idx_cont"]), "additive", "additive model")
    spec, theta, X, y, periods = periodic_case("Matern52", 1, 150, 2)
    with periodic_engine(spec, 1, periods, theta, X, y) as eng:
        eng.factorize()
        refuses(eng, X[:5], 2, "periodic", "periodic model")
    spec = O.make_spec(3, [0, 1], kind="ExpQuad", coreg=[(2, 3)])
    rng = np.random.default_rng(0)
    X = np.column_stack([rng.standard_normal((80, 2)), rng.integers(0, 3, 80)]).astype(float)
    theta = O.pack_theta(spec, [1.0, 1.2], 1.0, 0.2, coreg=[(0.3 * rng.standard_normal((3, 2)), np.ones(3))])
    with make_engine(spec, theta, X, rng.standard_normal(80)) as eng:
        eng.factorize()
        refuses(eng, X[:5], 2, "coregion tables", "categorical dimension")


def test_bad_arguments_are_refused_and_write_nothing(gpu):
    from gumbi_amd.engine import GMB_EINVAL

    spec, theta, X, y, inputs, _ = problem(300, 3, "Matern52", 16, 256)
    Xs = points(X, 50, [0, 1, 2])
    with make_engine(spec, theta, X, y) as eng:
        assert raw_prepare(eng, 4, 16, 3, 300) == GMB_EINVAL, "no factor"
        eng.factorize()
        before = eng.predict(Xs)
        for label, S, F, null in (("S = 0", 0, 16, ()), ("S = 513", 513, 16, ()), ("F = 0", 4, 0, ()), ("F = 16385", 4, 16385, ()),
                                  ("null omega", 4, 16, ("omega",)), ("null eps", 4, 16, ("eps",))):
            assert raw_prepare(eng, S, F, 3, 300, null) == GMB_EINVAL, label
            rc, _, clean = raw_eval(eng, Xs, S=4)
            assert rc == GMB_EINVAL and clean, f"{label}: evaluation after a refused preparation"
        eng.paths_prepare(*inputs)
        for label, kw in (("null Y", {"null": ("Y",)}), ("null Xs", {"null": ("Xs",)})):
            rc, _, clean = raw_eval(eng, Xs, **kw)
            assert rc == GMB_EINVAL and clean, label
        for label, draw in (("draw = S", [0] * 49 + [16]), ("draw < 0", [-1] + [0] * 49)):
            for form in (PACKED_HOST, STRIDED_DEVICE):
                rc, _, clean = raw_own(eng, Xs, draw, form)
                assert rc == GMB_EINVAL and clean, f"{label} ({form.name})"
            with pytest.raises(ValueError, match="outside"):
                eng.paths_eval_own(Xs, draw)
        rc, _, clean = raw_eval(eng, Xs[:0], STRIDED_HOST)  # (a leading dimension of its own: the packed one would be 0)
        assert rc == 0 and clean, "M == 0 is GMB_OK and writes nothing"
        after = eng.predict(Xs)
        assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
        assert raw_prepare(eng, 4, 16, 3, 300) == 0 and eng.n_paths == 4  # a set prepared past the binding: the engine's count sizes Y
        assert eng.paths_eval(Xs).shape == (4, 50)
        eng.set_dist_mode(eng.DIST_CAPACITY)
        assert raw_prepare(eng, 4, 16, 3, 300) == GMB_EINVAL, "capacity mode"
        assert "not available on distributed engines" in eng._lib.gmb_last_error(eng._h).decode()  # (not the missing factor's message)


@pytest.mark.parametrize("form", [STRIDED_HOST, STRIDED_DEVICE], ids=lambda f: f.name)
def test_device_memory_and_strided_forms(gpu, form):
    spec, theta, X, y, inputs, _ = problem(300, 3, "Matern52", 17, 1000)
    Xs = points(X, 333, [0, 1, 2], on_train=111)
    draw = np.arange(333) % 17
    with prepared(spec, theta, X, y, inputs) as eng:
        want = eng.paths_eval(Xs)
        w_val, w_grad = eng.paths_eval_own(Xs, draw)
        rc, got, _ = raw_eval(eng, Xs, form)
        assert rc == 0
        same_bits(got, want, f"{form.name} paths_eval")
        rc, (val, grad), _ = raw_own(eng, Xs, draw, form)
        assert rc == 0
        same_bits(val, w_val, f"{form.name} own values")
        same_bits(grad, w_grad, f"{form.name} own gradients")
        rc, (val, none), _ = raw_own(eng, Xs, draw, form, grad=False)
        assert rc == 0 and none is None
        same_bits(val, w_val, f"{form.name} own values without gradients")


# ---- 4. the front end -----------------------------------------------------------------------------------------------------------------
def test_frontend_draw_paths_and_propose_thompson(gpu):
    import gumbi_amd as gmb

    ds = frontend_dataset(300, ["y"])
    gp = gmb.GP(ds, outputs="y")
    gp.fit(continuous_dims=["a", "b"], MAP_kwargs={"maxeval": 25})
    gp.prepare_grid(resolution=12)
    paths = gp.draw_paths(4, n_features=256, seed=1)
    grid = paths.on_grid()
    assert grid.shape == (4, 12, 12)
    flat = paths.at_points(gp.grid_points)
    assert flat.shape == (4, 144)
    assert np.array_equal(np.asarray(flat.z.values()).reshape(4, 12, 12), np.asarray(grid.z.values()))
    assert np.all(np.isfinite(np.asarray(grid.z.values()))) and float(np.std(np.asarray(grid.z.values()), axis=0).max()) > 0.0
    z0 = np.zeros((3, 2))
    val, grad = paths.value_and_grad(z0, [0, 1, 3])
    assert val.shape == (3,) and grad.shape == (3, 2) and np.all(np.isfinite(grad))

    prop = gp.propose_thompson(5, num_restarts=3, raw_samples=64, n_features=256, seed=1, maxiter=30)
    assert prop is gp.proposal
    lo, hi = gp.optimization_bounds
    z = np.column_stack([prop[d].z.values().ravel() for d in gp.continuous_dims])
    assert z.shape == (5, 2) and np.all(z >= lo - 1e-12) and np.all(z <= hi + 1e-12)
    raw = gp.proposal_raw_acquisition
    own = np.asarray(gp.proposal_acquisition)
    print(f"proposal {z.tolist()}, own-draw values {own.tolist()}, best raw samples {raw.max(axis=1).tolist()}, {gp.proposal_result.nfev} evaluations")
    assert raw.shape == (5, 64) and own.shape == (5,)
    assert np.all(own >= raw.max(axis=1) - 1e-10 * np.abs(raw).max())  # (own-draw and all-draws values agree to 1e-10 relative)
    value, _ = gp.proposal_paths.value_and_grad(z, np.arange(5), grad=False)
    assert rel(value, own) <= 1e-10
    again = gp.propose_thompson(5, num_restarts=3, raw_samples=64, n_features=256, seed=1, maxiter=30)
    z2 = np.column_stack([again[d].z.values().ravel() for d in gp.continuous_dims])
    assert z2.tobytes() == z.tobytes()
    with pytest.raises(ValueError, match="stale"):  # the engine holds ONE set: propose_thompson has drawn others since
        paths.on_grid()
    with pytest.raises(ValueError, match="stale"):
        paths.value_and_grad(z0, [0, 1, 3])
    older, newer = gp.proposal_paths, gp.draw_paths(8, n_features=64, seed=2)
    with pytest.raises(ValueError, match="stale"):
        older.at_points(gp.grid_points)
    assert newer.at_points(gp.grid_points).shape == (8, 144)
    low = gp.propose_thompson(2, maximize=False, num_restarts=2, raw_samples=32, n_features=64, seed=2, maxiter=10)
    assert np.all(np.asarray(gp.proposal_acquisition) <= gp.proposal_raw_acquisition.min(axis=1) + 1e-10 * np.abs(gp.proposal_raw_acquisition).max())
    assert np.column_stack([low[d].z.values().ravel() for d in gp.continuous_dims]).shape == (2, 2)


def test_sparse_and_classification_front_ends_refuse(gpu):
    import gumbi_amd as gmb

    for cls in (gmb.SparseGP, gmb.GPC):
        for name in ("draw_paths", "propose_thompson"):
            assert name in cls.NOT_BUILT
            with pytest.raises(NotImplementedError, match=name):
                getattr(cls, name)(None)
